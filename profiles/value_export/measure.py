#!/usr/bin/env python3
"""Kernel times of the policy launch with the value export off, with nodes = 1 and with nodes = N + 1, and of sddp_value_at_device,
by events on the stream the handle shares with torch: the median of `--reps` launches behind one solve, one JSON line per shape.

    python profiles/value_export/measure.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from srbd_horizon_amd import workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402


def timed(eng, launch, reps):
    """per launch: the time between two events on the stream the handle shares with torch (DdpEngine.use_torch_stream)"""
    ms = []
    for _ in range(reps + 3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        launch()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms = np.array(ms[3:])
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for model, N, B in (("srbd13", 30, 1024), ("srbd61", 20, 512)):
        batch = workload.make_batch(model, N, np.arange(B))
        eng = DdpEngine(model, N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), consts=batch["consts"])
        eng.use_torch_stream()
        eng.enable_policy(1)
        eng.load(batch["x0"], batch["xs"], batch["us"])
        eng.solve(batch["params"])
        out = dict(model=model, N=N, B=B, reps=a.reps, policy_off=timed(eng, eng.policy_range_device, a.reps))
        for nodes in (1, N + 1):
            eng.enable_value(nodes)
            out[f"policy_nodes_{nodes}"] = timed(eng, eng.policy_range_device, a.reps)
        xm = torch.from_numpy(batch["x0"] + 1e-2).cuda()
        res = torch.empty((B, 8), dtype=torch.float64, device="cuda")
        out["value_at"] = timed(eng, lambda: eng.value_at_device(xm, res, 0), a.reps)
        eng.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
