#!/usr/bin/env python3
"""What the plan audit costs beside the solve it follows, on one handle.

    python profiles/plan_audit/measure.py [--reps 50] [--solves 5]

For srbd13 (N = 30) with 1024 and 20 480 robots and srbd37 (N = 20) with 512, workload.make_batch seeds 0 .. B - 1: the solve launch
from the warm start (load_range_device + solve_range_device; `--solves` launches after one warm-up, the load outside the timed region)
and the audit of the solved plans (audit_device; `--reps` launches after three warm-ups), each between two events on the handle's
stream.  Prints one JSON line per case: best and mean time of both in microseconds and the ratio of the best times."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from srbd_horizon_amd import _lib, workload  # noqa: E402

CASES = (("srbd13", 30, 1024), ("srbd13", 30, 20480), ("srbd37", 20, 512))


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
        out = torch.empty((B, _lib.AUDIT_WORDS), dtype=torch.float64, device="cuda")
        solve = timed(lambda: eng.solve_range_device(t["params"], 0, B), a.solves, 1, lambda: eng.load_range_device(0, B, t["x0"], t["xs"], t["us"]))
        audit = timed(lambda: eng.audit_device(out), a.reps, 3)
        rec = out.cpu().numpy()
        print(json.dumps(dict(model=model, N=N, count=B, solve_best_us=solve[0], solve_mean_us=solve[1], audit_best_us=audit[0], audit_mean_us=audit[1],
                              audit_over_solve=audit[0] / solve[0], outside_cone=float(np.mean(rec[:, _lib.AUDIT_CONE] > 0.0)),
                              pulling=float(np.mean(rec[:, _lib.AUDIT_PULL] > 0.0)), worst_defect=float(rec[:, _lib.AUDIT_DEFECT].max()))), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
