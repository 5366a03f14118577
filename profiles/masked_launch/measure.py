#!/usr/bin/env python3
"""What a masked launch costs beside the range launch, and a masked advance beside sddp_advance: 20 480 srbd13 instances (N = 30), the
time between two events on the stream the handle shares with torch around ONE launch sequence, the median of `--reps` launches after 3
discarded ones.  Every solve launch starts from the same reloaded warm start (the reload is outside the timed interval).  One JSON line
per queue order, and one for the advance.

    python profiles/masked_launch/measure.py [--reps 8] [--instances 20480]

selected = 0 is the pre-pass alone: the mask kernels, the key kernel and the sort where the order has them, and a solve kernel whose
workgroups find the queue empty.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from srbd_horizon_amd import workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402

FRACTIONS = (("all", 1.0), ("1/2", 0.5), ("1/4", 0.25), ("1/16", 0.0625), ("none", 0.0))


def timed(launch, reps, before=None):
    ms = []
    for _ in range(reps + 3):
        if before is not None:
            before()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        launch()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms = np.array(ms[3:])
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4), max_ms=round(float(ms.max()), 4))


def mask_of(B, frac, seed=0):
    m = np.zeros(B, np.int32)
    m[np.random.default_rng(seed).permutation(B)[:int(round(frac * B))]] = 1
    return torch.from_numpy(m).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--instances", type=int, default=20480)
    a = ap.parse_args()
    model, N, B = "srbd13", 30, a.instances
    batch = workload.make_batch(model, N, np.arange(B))
    dev = {k: torch.from_numpy(np.ascontiguousarray(batch[k])).cuda() for k in ("x0", "xs", "us", "params")}
    masks = {name: mask_of(B, f) for name, f in FRACTIONS}
    for order in (0, 1, 2):
        eng = DdpEngine(model, N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3, waves_per_simd=2, queue_order=order),
                        consts=batch["consts"])
        eng.use_torch_stream()
        reload = lambda: eng.load_range_device(0, B, dev["x0"], dev["xs"], dev["us"])      # noqa: E731
        reload()
        eng.solve_range_device(dev["params"], 0, B)                                         # (fills the previous iteration counts)
        out = dict(what="solve", model=model, N=N, B=B, queue_order=order, reps=a.reps, slots=eng.queue_info()[0],
                   range=timed(lambda: eng.solve_range_device(dev["params"], 0, B), a.reps, reload))
        for name, _ in FRACTIONS:
            out["masked " + name] = dict(timed(lambda: eng.solve_masked_device(dev["params"], masks[name]), a.reps, reload),
                                         selected=eng.last_selected())
        eng.close()
        print(json.dumps(out), flush=True)
    # the advance: sddp_advance takes host rows of the whole batch (its upload is part of the call), the masked form device rows
    eng = DdpEngine(model, N, B, opts=dict(max_iters=0), consts=batch["consts"])
    eng.use_torch_stream()
    eng.set_params(batch["params"])
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve_resident()
    p_last, x0 = np.ascontiguousarray(batch["params"][:, N]), np.ascontiguousarray(batch["x0"])
    d_pl, d_x0 = torch.from_numpy(p_last).cuda(), torch.from_numpy(x0).cuda()
    out = dict(what="advance", model=model, N=N, B=B, reps=a.reps, host_sddp_advance=timed(lambda: eng.advance(p_last, x0), a.reps))
    t = time.perf_counter()
    for _ in range(a.reps):
        eng.advance(p_last, x0)
    eng.synchronize()
    out["host_sddp_advance_wall_ms"] = round(1e3 * (time.perf_counter() - t) / a.reps, 4)
    for name, _ in FRACTIONS:
        out["masked " + name] = timed(lambda: eng.advance_masked_device(masks[name], d_pl, d_x0), a.reps)
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
