#!/usr/bin/env python3
"""Time-budgeted launches: what the budget costs while it is not armed, and how far an armed launch overruns its deadline.

    python profiles/deadline/measure.py --cost    [--launches 5]     one JSON line; run it with SDDP_LIB pointing at the parent's
                                                                     library and at this tree's, alternately (README.md)
    python profiles/deadline/measure.py --overrun [--points 10]      one JSON line per shape

Shapes: srbd13, N = 30, 20 480 instances (the 1024 bench instances, workload.make_batch seeds 0..1023, 20 times over),
waves_per_simd = 2; srbd37, N = 20, 2 048 instances (seeds 0..255, 8 times over), waves_per_simd = 2.  Every launch runs on a handle
with sddp_enable_resume, queue_order = 0, the batch loaded before it; times are the HIP-event time of the launch
(sddp_last_kernel_ms).
--cost: no budget is ever armed (the parent's library has none): kernel_ms of `--launches` launches after one warm-up launch.
--overrun: T = median of 3 uncut launches; then budgets T * (i + 0.5) / points, min_iters 0 and 1: instances cut, the overrun
  (latest slot end minus deadline, sddp_device_ptr 7 and 11) and, to compare it with, one iteration's time
  T * slots / (instances * mean iterations)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from srbd_horizon_amd import _lib, workload  # noqa: E402

import torch  # noqa: E402,F401  (its HIP runtime first, as _lib.load does)

if not hasattr(__import__("ctypes").CDLL(_lib.LIB_PATH), "sddp_set_time_budget"):      # a parent library (--cost): no budget functions
    _lib.SYMBOLS.pop("sddp_set_time_budget"); _lib.SYMBOLS.pop("sddp_time_budget_info")
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3, waves_per_simd=2, queue_order=0)
SHAPES = (("srbd13", 30, 1024, 20), ("srbd37", 20, 256, 8))


def make(model, N, seeds, times):
    b = workload.make_batch(model, N, np.arange(seeds))
    t = {k: np.ascontiguousarray(np.concatenate([b[k]] * times)) for k in ("x0", "xs", "us", "params")}
    eng = DdpEngine(model, N, seeds * times, opts=OPTS, consts=b["consts"])
    eng.enable_resume()
    eng.enable_timing()
    eng.set_params(t["params"])

    def launch():
        eng.set_initial_state(t["x0"]); eng.set_x_warmstart(t["xs"]); eng.set_u_warmstart(t["us"])
        eng.solve_resident_first()
        eng.synchronize()
        return eng.last_kernel_ms()

    return eng, launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--overrun", action="store_true")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--points", type=int, default=10)
    args = ap.parse_args()
    for model, N, seeds, times in SHAPES:
        eng, launch = make(model, N, seeds, times)
        launch()
        if args.cost:
            ms = [round(launch(), 4) for _ in range(args.launches)]
            print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "model": model, "N": N, "instances": seeds * times, "kernel_ms": ms}), flush=True)
        if args.overrun:
            T = statistics.median(launch() for _ in range(3))
            iters = eng.first_stats["iters"]
            slots = eng.queue_info()[1]
            one_iter_us = 1e3 * T * slots / (len(iters) * float(iters.mean()))
            rows = []
            for mi in (0, 1):
                for i in range(args.points):
                    budget = 1e3 * T * (i + 0.5) / args.points
                    eng.set_time_budget(budget, mi)
                    ms = launch()
                    rows.append(dict(min_iters=mi, budget_us=round(budget, 1), launch_us=round(1e3 * ms, 1),
                                     overrun_us=round(eng.deadline_overrun_us(), 1), cut=int((eng.first_stats["status"] == 1).sum())))
                eng.set_time_budget(0.0)
            print(json.dumps({"model": model, "N": N, "instances": seeds * times, "slots": slots, "T_uncut_us": round(1e3 * T, 1),
                              "mean_iters": round(float(iters.mean()), 2), "one_iteration_us": round(one_iter_us, 1), "sweep": rows}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
