#!/usr/bin/env python3
"""A fleet tick in two slices: hand out the finished robots after 6 iterations, then finish the stragglers alone
(include/sddp.h: sddp_enable_resume, sddp_continue_range_device).

    python examples/time_sliced_fleet.py [--robots 1024] [--first-slice 6] [--horizon 30]

A launch ends with its slowest instance.  `--robots` cold-started srbd13 MPC instances run for at most `--first-slice` iterations
in one launch; the first-knot records of the ones that are finished then are final.  A second launch takes up only the unfinished
solves where they stopped.  Every robot ends with exactly the result of the uncut solve, which the example checks byte for byte
against a second handle that never slices.  Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402
from srbd_horizon_amd.fleet import FleetQueue  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--first-slice", type=int, default=6)
    ap.add_argument("--horizon", type=int, default=30)
    args = ap.parse_args()
    R, N, k, total = args.robots, args.horizon, args.first_slice, 100
    dev = torch.device("cuda", 0)
    opts = dict(max_iters=total, alpha_converge_threshold=1e-12, beta=1e-3, waves_per_simd=2)
    b = workload.make_batch("srbd13", N, np.arange(R))
    d = {n: torch.from_numpy(b[n]).to(dev) for n in ("x0", "xs", "us", "params")}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    results = {}
    for name in ("uncut", "sliced"):
        eng = DdpEngine("srbd13", N, R, opts=opts, consts=b["consts"])
        fleet = FleetQueue(eng, d["params"], R, 1)
        for rep in range(2):                                             # the second pass is the timed one
            fleet.submit(d["x0"], d["xs"], d["us"])
            if name == "uncut":
                _, ms = timed(fleet.flush)
            else:
                (finished, records), ms = timed(lambda: fleet.solve_sliced(k, total))
        x, u, st = eng.fetch()
        results[name] = (x.copy(), u.copy(), st.copy(), ms)
        if name == "sliced":
            n_fin = int(finished.sum().item())
            print(f"{R} robots, first slice {k} iterations: {n_fin} finished ({100.0 * n_fin / R:.1f} %), "
                  f"{R - n_fin} continued in a second launch; both slices {ms:.2f} ms (uncut launch {results['uncut'][3]:.2f} ms)")
        eng.close()
    same = all(results["uncut"][i].tobytes() == results["sliced"][i].tobytes() for i in range(3))
    it = results["uncut"][2]["iters"]
    print(f"iterations of the uncut solves: mean {it.mean():.1f}, max {it.max()}")
    print("every result (xs, us, stats) equals the uncut solve, byte for byte" if same else "MISMATCH between the sliced and the uncut solve")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
