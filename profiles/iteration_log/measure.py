#!/usr/bin/env python3
"""The price of the iteration log: HIP-event time of the solve launch on the same handle and batch with resumable solves enabled,
log off against log on (2 warm-up + 7 timed launches each, median and min-max), and the resources of the kernels that ran.

    python profiles/iteration_log/measure.py > profiles/iteration_log/measure.json

Batches: srbd13 N = 30, 20 480 instances, waves_per_simd 2; srbd37 N = 20, 2 048 instances."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from srbd_horizon_amd import workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402

ROWS = 128


def times(eng, b, reps=9, warm=2):
    ms = []
    for _ in range(reps):
        eng.set_initial_state(b["x0"]); eng.set_x_warmstart(b["xs"]); eng.set_u_warmstart(b["us"])
        eng.solve(b["params"])
        ms.append(eng.last_kernel_ms())
    ms = np.array(ms[warm:])
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()))


def main():
    out = []
    for model, N, B, wps in (("srbd13", 30, 20480, 2), ("srbd37", 20, 2048, 1)):
        b = workload.make_batch(model, N, list(range(B)))
        eng = DdpEngine(model, N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3, waves_per_simd=wps), consts=b["consts"])
        eng.enable_timing(True)
        eng.enable_resume()
        row = dict(model=model, N=N, B=B, waves_per_simd=wps)
        row["log_off"] = dict(times(eng, b), resources=eng.kernel_info())
        st_off = eng.stats.copy()
        eng.enable_iteration_log(ROWS)
        row["log_on"] = dict(times(eng, b), resources=eng.kernel_info())
        rec, n = eng.iteration_log()
        row["identical_stats"] = bool(eng.stats.tobytes() == st_off.tobytes())
        row["records"] = int(n.sum()); row["saturated"] = int((n == ROWS).sum())
        row["ratio"] = row["log_on"]["median"] / row["log_off"]["median"]
        eng.close()
        out.append(row)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
