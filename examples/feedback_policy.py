#!/usr/bin/env python3
"""The srbd37 walking loop with a force disturbance, first input applied open loop vs. the solver's feedback policy.

    python examples/feedback_policy.py [--ticks 20] [--substeps 4] [--push 2.0]

Every tick's simulator step is split into `--substeps` Euler sub-steps; a lateral force (`--push`, as a CoM acceleration in m/s^2,
unknown to the solver) acts over ticks 6..9.  Open loop applies u_0 at every sub-step; the policy applies u_0 + K_0 (x - x_0) with the
first knot's gain of the RETURNED iterate (DDPSolver.get_feedback_gains, sddp_policy_range_device).  Prints the peak lateral CoM
deviation from the undisturbed run of each mode.  Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd.mpc import MpcLoop  # noqa: E402


def run(ticks, substeps, feedback, push):
    loop = MpcLoop("srbd37", 20, feedback_substeps=substeps, feedback=feedback)
    y = []
    for t in range(ticks):
        loop.tick("walking", (1.0, 0.0), push=(0.0, push, 0.0) if (push and 6 <= t <= 9) else None)
        y.append(loop.state[1])
    return np.array(y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--substeps", type=int, default=4)
    ap.add_argument("--push", type=float, default=2.0)
    a = ap.parse_args()
    for name, fb in (("open loop", False), ("policy", True)):
        dev = np.abs(run(a.ticks, a.substeps, fb, a.push) - run(a.ticks, a.substeps, fb, 0.0))
        print(f"{name:9s}: peak lateral CoM deviation {dev.max():.5f} m (tick {int(dev.argmax())})")


if __name__ == "__main__":
    main()
