#!/usr/bin/env python3
"""Which way to move the next foothold: the gradient of a plan's cost in its parameters, on the device.

    python examples/foothold_gradient.py [--robots 1024] [--step 0.005]

`--robots` srbd13 robots (N = 30) are solved once.  On srbd13 the contact points are parameters (columns 11 .. 16 of a parameter row),
placed by a fixed stride heuristic; sddp_param_gradient_range_device gives d cost / d P for every node.  For each robot whose plan has
a foot in the air at node 0, the touchdown foothold of that foot is the x, y of its contact point on every node from touchdown on, and
the gradient in it is the sum of G over those nodes.  The foothold is moved `--step` metres against that gradient and the fleet is
solved again.  Printed: the share of robots whose converged cost fell, and the predicted change G . dp against the actual change.
The prediction is first order and holds where the plan is converged with closed gaps (record words "stationarity", "defect").
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
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--step", type=float, default=0.005)
    a = ap.parse_args()
    N, B = 30, a.robots
    batch = workload.make_batch("srbd13", N, np.arange(B))
    P = batch["params"].copy()
    eng = DdpEngine("srbd13", N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), consts=batch["consts"])
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(P)
    cost0, ok0 = eng.stats["cost"].copy(), eng.stats["converged"].astype(bool)
    grad, rec = eng.param_gradient()
    eng.synchronize()
    G = grad.cpu().numpy()
    dP = np.zeros_like(P)
    moved = np.zeros(B, dtype=bool)
    for b in range(B):
        sw = P[b, :, 17:19] > 0.5                                   # [node, foot]: in stance
        for foot in range(2):
            down = np.flatnonzero(sw[:, foot])
            if sw[0, foot] or down.size == 0:
                continue                                            # not the swing foot, or it never lands inside the horizon
            cols = slice(11 + 3 * foot, 13 + 3 * foot)              # x, y of the contact point
            g = G[b, down[0]:, cols].sum(axis=0)
            if np.linalg.norm(g) > 0.0:
                dP[b, down[0]:, cols] = -a.step * g / np.linalg.norm(g)
                moved[b] = True
    predicted = np.sum(G * dP, axis=(1, 2))
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(P + dP)
    cost1, ok = eng.stats["cost"].copy(), ok0 & eng.stats["converged"].astype(bool) & moved
    eng.close()
    actual = cost1 - cost0
    print(f"{int(moved.sum())} of {B} robots have a foot in the air at node 0 that lands inside the horizon; {int(ok.sum())} of them converged twice")
    if ok.any():
        ratio = actual[ok] / predicted[ok]
        print(f"cost fell on {100.0 * np.mean(actual[ok] < 0.0):.1f} % of them (foothold moved {1e3 * a.step:.1f} mm against the gradient)")
        print(f"actual / predicted change of the cost: median {np.median(ratio):.3f}, 10 % .. 90 % {np.quantile(ratio, 0.1):.3f} .. {np.quantile(ratio, 0.9):.3f}")
        print(f"mean predicted {predicted[ok].mean():.4e}, mean actual {actual[ok].mean():.4e}")


if __name__ == "__main__":
    main()
