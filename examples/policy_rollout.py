#!/usr/bin/env python3
"""Where a pushed fleet goes under the previous plan's policy: the closed-loop prediction on the device, beside the open-loop one.

    python examples/policy_rollout.py [--robots 1024] [--push 0.2] [--knots 4]

`--robots` srbd13 robots are solved once (N = 30) with the policy of the first `--knots` knots exported.  Every robot is then pushed:
its measured state is x_0 + delta, delta a lateral CoM velocity of `--push` m/s.  sddp_policy_rollout_device predicts the next
`--knots` knots through the solver's own model with u_k + K_k (x - x_k); the same call on a second handle that solved the same
problems but never ran its policy launch (ok = 0) gives the open-loop rollout of u_k from the same states.  Prints the fleet's
median and worst lateral deviation from the plan at the last knot, for both.  Needs a GPU: the engine has no CPU fallback.
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
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--push", type=float, default=0.2)
    ap.add_argument("--knots", type=int, default=4)
    a = ap.parse_args()
    N, B, M = 30, a.robots, a.knots
    batch = workload.make_batch("srbd13", N, np.arange(B))
    opts = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
    dev = {}
    for name, feedback in (("closed loop", True), ("open loop", False)):
        eng = DdpEngine("srbd13", N, B, opts=opts, consts=batch["consts"])
        eng.enable_policy(M)
        eng.load(batch["x0"], batch["xs"], batch["us"])
        x, _ = eng.solve(batch["params"])
        if feedback:
            eng.policy_range_device()
        x_meas = x[:, 0].copy()
        x_meas[:, 8] += a.push                                   # x = r | o | rdot | w: the lateral CoM velocity
        xr, _, _ = eng.policy_rollout(x_meas)
        dev[name] = np.abs(xr[:, M, 1] - x[:, M, 1])
        eng.close()
    for name, d in dev.items():
        print(f"{name:11s}: lateral CoM deviation from the plan at knot {M} over {B} robots: median {np.median(d):.5f} m, worst {d.max():.5f} m")


if __name__ == "__main__":
    main()
