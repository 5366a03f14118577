#!/usr/bin/env python3
"""What the stationarity certificate costs beside the solve it follows, on one handle (the method of profiles/plan_audit/measure.py).

    python profiles/stationarity/measure.py [--reps 50] [--solves 5]

For srbd13 (N = 30) with 1024 robots and srbd37 (N = 20) with 512, workload.make_batch seeds 0 .. B - 1: the solve launch from the warm
start (load_range_device + solve_range_device; `--solves` launches after one warm-up, the load outside the timed region), the
certificate of the solved plans (stationarity_device, record alone and with both full outputs; `--reps` launches after three warm-ups)
and the plan audit, each between two events on the handle's stream.  Prints one JSON line per case: best and mean times in microseconds."""
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
        out, lam, grad, aud = mk(len(_lib.STATIONARITY_FIELDS)), mk(N + 1, eng.nx), mk(N, eng.nu), mk(_lib.AUDIT_WORDS)
        solve = timed(lambda: eng.solve_range_device(t["params"], 0, B), a.solves, 1, lambda: eng.load_range_device(0, B, t["x0"], t["xs"], t["us"]))
        rec = timed(lambda: eng.stationarity_device(out), a.reps, 3)
        full = timed(lambda: eng.stationarity_device(out, lam=lam, grad=grad), a.reps, 3)
        audit = timed(lambda: eng.audit_device(aud), a.reps, 3)
        r = out.cpu().numpy()
        rel = r[:, 0] / r[:, 3]
        print(json.dumps(dict(model=model, N=N, count=B, solve_best_us=solve[0], solve_mean_us=solve[1], record_best_us=rec[0], record_mean_us=rec[1],
                              full_best_us=full[0], full_mean_us=full[1], audit_best_us=audit[0], record_over_solve=rec[0] / solve[0],
                              relative_median=float(np.median(rel)), relative_max=float(rel.max()))), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
