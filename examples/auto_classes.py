#!/usr/bin/env python3
"""A receding-horizon fleet on queue_order = 3 that never passes a class label (include/sddp.h: sddp_enable_auto_classes,
sddp_get_class_stats / sddp_add_class_stats).

    python examples/auto_classes.py [--robots 8192] [--ticks 6] [--horizon 30]

Every tick shifts the resident parameters by one knot on the device (sddp_advance), so every robot's gait phase -- and with it the
class of its problem -- changes every tick.  The handle labels the instances of each launch itself, from the parameters the launch
runs on, learns the mean iteration count of every class and starts the long classes first; the example prints how many labels
changed from tick to tick and checks them against the numpy statement of the formula (workload.schedule_classes).  The ids are the
library's own, so the learned history means something to another handle: a second, fresh handle is seeded with the first one's
history and orders its FIRST launch by it, where the first handle had to start in initial-cost order.
Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=6)
    ap.add_argument("--horizon", type=int, default=30)
    args = ap.parse_args()
    R, N, T = args.robots, args.horizon, args.ticks
    opts = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3, waves_per_simd=2, queue_order=3)
    # the gait schedule and commands of a longer horizon: its window [t, t + N] is the fleet's parameter tensor at tick t
    long = workload.make_batch("srbd13", N + T, np.arange(R))
    P_long = long["params"]

    def handle():
        eng = DdpEngine("srbd13", N, R, opts=opts, consts=long["consts"])
        eng.enable_auto_classes()                                         # no label is ever passed
        eng.enable_timing()
        eng.set_params(P_long[:, :N + 1])
        eng.load(long["x0"], long["xs"][:, :N + 1], long["us"][:, :N])
        return eng

    ok = True
    fleet = handle()
    print(f"{R} robots, N = {N}, {fleet.auto_classes_info()[1]} classes; slots {fleet.queue_info()[0]}")
    prev = cold_ms = None
    for t in range(T):
        if t:
            fleet.advance(P_long[:, t + N], x1)                           # shift on the device; the plan's next state is the new x0
        u0, x1 = fleet.solve_resident_first()
        fleet.synchronize()
        labels = fleet.instance_classes()
        ok &= bool(np.array_equal(labels, workload.schedule_classes("srbd13", P_long[:, t:t + N + 1])[0]))
        moved = "" if prev is None else f", {int((labels != prev).sum())} robots changed class"
        it = fleet.first_stats["iters"]
        print(f"tick {t}: {len(np.unique(labels))} classes present{moved}; iterations mean {it.mean():.1f} max {it.max()}; "
              f"launch {fleet.last_kernel_ms():.2f} ms")
        cold_ms = fleet.last_kernel_ms() if t == 0 else cold_ms
        prev = labels
    stats = fleet.class_stats()
    print(f"history learned: {int((stats[:, 1] > 0).sum())} classes, {int(stats[:, 1].sum())} solves")
    seeded = handle()                                                     # e.g. the server after a restart
    seeded.add_class_stats(stats)
    seeded.solve_resident_first()
    seeded.synchronize()
    print(f"first launch of a fresh handle on tick 0's problems: {cold_ms:.2f} ms without history (initial-cost order), "
          f"{seeded.last_kernel_ms():.2f} ms seeded with the first handle's history")
    print("device labels equal workload.schedule_classes at every tick" if ok else "MISMATCH between device and numpy labels")
    fleet.close(); seeded.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
