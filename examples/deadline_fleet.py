#!/usr/bin/env python3
"""A fleet tick under a time budget: the launch ends at a device-clock deadline, the robots that are finished then are handed out,
the stragglers are finished alone (include/sddp.h: sddp_set_time_budget, sddp_continue_range_device).

    python examples/deadline_fleet.py [--robots 1024] [--budget-us 1000] [--min-iters 0] [--horizon 30]

examples/time_sliced_fleet.py cuts the first launch after a number of iterations, which somebody has to guess per model, horizon and
GPU load.  A controller knows its slot in time: here `--robots` cold-started srbd13 MPC instances run in one launch that ends
`--budget-us` microseconds of device time after it started (every robot it runs gets at least `--min-iters` iterations); the
first-knot records of the robots that are finished then are final.  A second launch, with the budget off, takes up only the unfinished
solves where they stopped.  Every robot ends with exactly the result of the uncut solve, which the example checks byte for byte
against a second handle that never cuts.  Needs a GPU: the engine has no CPU fallback.
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
    ap.add_argument("--budget-us", type=float, default=1000.0)
    ap.add_argument("--min-iters", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=30)
    args = ap.parse_args()
    R, N, total = args.robots, args.horizon, 100
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
    for name in ("uncut", "budgeted"):
        eng = DdpEngine("srbd13", N, R, opts=opts, consts=b["consts"])
        fleet = FleetQueue(eng, d["params"], R, 1)
        for rep in range(2):                                             # the second pass is the timed one
            fleet.submit(d["x0"], d["xs"], d["us"])
            if name == "uncut":
                _, ms = timed(fleet.flush)
            else:
                (finished, records), ms = timed(lambda: fleet.solve_within(args.budget_us, total, args.min_iters))
        x, u, st = eng.fetch()
        results[name] = (x.copy(), u.copy(), st.copy(), ms)
        if name == "budgeted":
            n_fin = int(finished.sum().item())
            print(f"{R} robots, budget {args.budget_us:.0f} us (min_iters {args.min_iters}): {n_fin} finished inside it "
                  f"({100.0 * n_fin / R:.1f} %), {R - n_fin} continued in a second launch")
            print(f"the budgeted launch ended {fleet.overrun_us:.1f} us past its deadline; both launches {ms:.2f} ms on the host clock "
                  f"(uncut launch {results['uncut'][3]:.2f} ms)")
        eng.close()
    same = all(results["uncut"][i].tobytes() == results["budgeted"][i].tobytes() for i in range(3))
    it = results["uncut"][2]["iters"]
    print(f"iterations of the uncut solves: mean {it.mean():.1f}, max {it.max()}")
    print("every result (xs, us, stats) equals the uncut solve, byte for byte" if same else "MISMATCH between the budgeted and the uncut solve")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
