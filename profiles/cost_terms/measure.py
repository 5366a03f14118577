#!/usr/bin/env python3
"""What the cost breakdown costs beside the solve it follows, on one handle (the method of profiles/stationarity/measure.py).

    python profiles/cost_terms/measure.py [--reps 50] [--solves 5]

For srbd13 (N = 30) with 1024 robots and srbd37 (N = 20) with 512, workload.make_batch seeds 0 .. B - 1: the solve launch from the warm
start (load_range_device + solve_range_device; `--solves` launches after one warm-up, the load outside the timed region), the
breakdown of the solved plans (cost_terms_device, record alone and with the per-node addends; `--reps` launches after three warm-ups),
the stationarity certificate and the plan audit, each between two events on the handle's stream.  Prints one JSON line per case: best
and mean times in microseconds, and the fleet-mean share of every family."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from srbd_horizon_amd import _lib, workload  # noqa: E402

CASES = (("srbd13", 30, 1024), ("srbd37", 20, 512))


def timed(call, reps, warm, before=None):
    import torch
    t = []
    for i in range(warm + reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        e1.synchronize()
        if i >= warm:
            t.append(1e3 * e0.elapsed_time(e1))
    return min(t), float(np.mean(t))


def main():
    import torch
    from srbd_horizon_amd.engine import DdpEngine
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--solves", type=int, default=5)
    a = ap.parse_args()
    for model, N, B in CASES:
        batch = workload.make_batch(model, N, np.arange(B))
        eng = DdpEngine(model, N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), consts=batch["consts"])
        eng.use_torch_stream()
        t = {k: torch.from_numpy(batch[k]).cuda() for k in ("x0", "xs", "us", "params")}
        mk = lambda *s: torch.empty((B, *s), dtype=torch.float64, device="cuda")      # noqa: E731
        out, nodes = mk(_lib.COST_TERMS_WORDS), mk(N + 1, _lib.COST_TERMS_COLS)
        stat, aud = mk(len(_lib.STATIONARITY_FIELDS)), mk(_lib.AUDIT_WORDS)
        solve = timed(lambda: eng.solve_range_device(t["params"], 0, B), a.solves, 1, lambda: eng.load_range_device(0, B, t["x0"], t["xs"], t["us"]))
        rec = timed(lambda: eng.cost_terms_device(out), a.reps, 3)
        full = timed(lambda: eng.cost_terms_device(out, nodes=nodes), a.reps, 3)
        st = timed(lambda: eng.stationarity_device(stat), a.reps, 3)
        audit = timed(lambda: eng.audit_device(aud), a.reps, 3)
        r = out.cpu().numpy()
        share = (r[:, 1:14] / r[:, :1]).mean(axis=0)
        print(json.dumps(dict(model=model, N=N, count=B, solve_best_us=solve[0], solve_mean_us=solve[1], record_best_us=rec[0], record_mean_us=rec[1],
                              nodes_best_us=full[0], nodes_mean_us=full[1], stationarity_best_us=st[0], audit_best_us=audit[0],
                              record_over_solve=rec[0] / solve[0], nodes_over_solve=full[0] / solve[0],
                              total_minus_stats_cost_rel_max=float(np.max(np.abs(r[:, 0] - eng.fetch()[2]["cost"]) / np.abs(r[:, 0]))),
                              mean_share={n: float(s) for n, s in zip(_lib.COST_TERM_NAMES, share)})), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
