#!/usr/bin/env python3
"""Which plans of a fleet push harder than the ground allows or pull on a foot: the plan audit on the device.

    python examples/plan_audit.py [--robots 1024] [--push 0.2] [--knots 4] [--barrier 6.0] [--sharpness 30.0]

`--robots` srbd13 robots are solved once (N = 30), with the friction barrier off (the default, as in the reference) and on (weight
`--barrier`, sharpness `--sharpness`).  sddp_audit gives 16 words per robot; printed are the share of plans outside the friction
cone (word 0 > 0) or pulling on a stance foot (word 3 > 0), and the fleet's worst of each.  The barrier-off fleet is then pushed (a
lateral CoM velocity of
`--push` m/s), sddp_policy_rollout_device predicts `--knots` knots under the previous plan's policy, and the same audit is applied to
that prediction without fetching it.  Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import _lib, workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402


def report(name, rec):
    cone, pull = rec[:, _lib.AUDIT_CONE], rec[:, _lib.AUDIT_PULL]
    print(f"{name:30s}: outside the cone {np.mean(cone > 0.0):6.1%} (worst {cone.max():+.4f}), pulling {np.mean(pull > 0.0):6.1%} "
          f"(worst {pull.max():+.4f}), either {np.mean((cone > 0.0) | (pull > 0.0)):6.1%}; swing load {rec[:, _lib.AUDIT_SWING_LOAD].max():.4f}, "
          f"defect {rec[:, _lib.AUDIT_DEFECT].max():.1e}   [force_scaling N]")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--push", type=float, default=0.2)
    ap.add_argument("--knots", type=int, default=4)
    ap.add_argument("--barrier", type=float, default=6.0)
    ap.add_argument("--sharpness", type=float, default=30.0)
    a = ap.parse_args()
    N, B, M = 30, a.robots, a.knots
    batch = workload.make_batch("srbd13", N, np.arange(B))
    opts = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
    for name, consts in (("barrier off", batch["consts"]),
                         ("barrier on", dict(batch["consts"], friction_barrier_weight=a.barrier, friction_barrier_sharpness=a.sharpness))):
        eng = DdpEngine("srbd13", N, B, opts=opts, consts=consts)
        eng.load(batch["x0"], batch["xs"], batch["us"])
        eng.solve(batch["params"])
        print(f"{name}: {int(eng.stats['converged'].sum())} of {B} plans converged")
        report(name, eng.audit())
        eng.close()
    eng = DdpEngine("srbd13", N, B, opts=opts, consts=batch["consts"])
    eng.enable_policy(M)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, _ = eng.solve(batch["params"])
    eng.policy_range_device()
    x_meas = x[:, 0].copy()
    x_meas[:, 8] += a.push                                       # x = r | o | rdot | w: the lateral CoM velocity
    mk = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")      # noqa: E731
    xr, ur, rec = mk(B, M + 1, eng.nx), mk(B, M, eng.nu), mk(B, _lib.AUDIT_WORDS)
    eng.policy_rollout_device(torch.from_numpy(x_meas).cuda(), xr, ur)
    eng.audit_device(rec, x=xr, u=ur, start=0, steps=M)          # behind the rollout on the handle's stream: nothing is fetched but the record
    eng.synchronize()
    report(f"pushed, policy, {M} knots", rec.cpu().numpy())
    own = eng.audit()
    print(f"(the first {M} knots lie inside the plan, whose own audit over all {N} knots gives: outside the cone {np.mean(own[:, 0] > 0.0):.1%})")
    eng.close()


if __name__ == "__main__":
    main()
