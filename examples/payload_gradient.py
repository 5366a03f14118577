#!/usr/bin/env python3
"""Whose payload estimate matters: the gradient of every plan's cost in the robot's mass, on the device.

    python examples/payload_gradient.py [--robots 1024] [--horizon 30] [--step 0.01]

The fleet of examples/heterogeneous_fleet.py: `--robots` srbd13 robots that carry a payload of 0 - 25 % of the body mass (mass and
inertia scaled with it), every one with its own constants in one handle (sddp_set_instance_consts).  They are solved once;
sddp_const_gradient_range_device gives the gradient of every plan's cost in the derived constants, and sddp_const_gradient_fields, with
each robot's own constants, the gradient in the fields a user sets.  Printed: d cost / d m by payload quartile, and which constant
each plan is relatively most sensitive to.  Then every mass is raised by `--step` of itself, the fleet is solved again from the first
plans, and the predicted change  d cost / d m  x  delta m  is compared with the actual one.  The prediction is first order and holds
where the plan is converged with closed gaps (record words "stationarity", "defect").  Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import _lib, workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--step", type=float, default=0.01)
    a = ap.parse_args()
    N, B = a.horizon, a.robots
    batch = workload.make_batch("srbd13", N, np.arange(B))
    eng = DdpEngine("srbd13", N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), consts=batch["consts"])
    payload = np.random.default_rng(0).uniform(0.0, 0.25, B)         # fraction of the body mass
    I0 = np.asarray(list(eng.consts.I)).reshape(3, 3)
    mass = eng.consts.m * (1.0 + payload)
    inertia = I0[None] * (1.0 + payload)[:, None, None]
    eng.set_instance_consts({"m": mass, "I": inertia})
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    cost0, ok0 = eng.stats["cost"].copy(), eng.stats["converged"].astype(bool)
    rec, fields = eng.const_gradient()
    dJdm = np.array([f["m"] for f in fields])
    names = _lib.CONST_GRADIENT_NAMES
    edges = np.quantile(payload, [0.0, 0.25, 0.5, 0.75, 1.0])
    print(f"{B} robots, payload 0 - 25 % of {eng.consts.m:.0f} kg; gradient of each plan's cost in its own mass:")
    for q in range(4):
        sel = (payload >= edges[q]) & ((payload < edges[q + 1]) | (q == 3))
        print(f"  payload {100 * edges[q]:4.1f} - {100 * edges[q + 1]:4.1f} %: d cost / d m mean {dJdm[sel].mean():+.4e} per kg, "
              f"largest |.| {np.abs(dJdm[sel]).max():.4e}")
    top = rec[:, 33].astype(int)
    for c in np.unique(top[top >= 0]):
        print(f"  {int((top == c).sum()):5d} plans are relatively most sensitive to {names[c]}")
    dm = a.step * mass
    eng.set_instance_consts({"m": mass + dm, "I": inertia})
    eng.load(batch["x0"], x, u)
    eng.solve(batch["params"])
    cost1, ok = eng.stats["cost"].copy(), ok0 & eng.stats["converged"].astype(bool)
    eng.close()
    predicted, actual = dJdm * dm, cost1 - cost0
    if ok.any():
        ratio = actual[ok] / predicted[ok]
        print(f"every mass raised by {100 * a.step:.1f} %; {int(ok.sum())} robots converged twice")
        print(f"actual / predicted change of the cost: median {np.median(ratio):.3f}, 10 % .. 90 % {np.quantile(ratio, 0.1):.3f} .. {np.quantile(ratio, 0.9):.3f}")
        print(f"mean predicted {predicted[ok].mean():+.4e}, mean actual {actual[ok].mean():+.4e}")


if __name__ == "__main__":
    main()
