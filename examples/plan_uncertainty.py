#!/usr/bin/env python3
"""How much state-estimate and actuation noise a fleet's plans absorb before a stance foot leaves its friction cone: the closed-loop
covariance of every plan under its exported policy, on the device.

    python examples/plan_uncertainty.py [--robots 1024] [--pos 0.005] [--vel 0.05] [--att 0.01] [--r 1e-4] [--r-large 1e-2]

`--robots` srbd13 robots are solved once (N = 30, the friction barrier off) with all N knots of the policy exported.  The estimate's
noise is Sigma0 = diag: standard deviations `--pos` m on the CoM position, `--att` on every quaternion entry, `--vel` m/s on the CoM
velocity and `--vel` rad/s on the angular velocity.  sddp_policy_covariance_device propagates it along every plan; printed are the
histogram of word 0 (the smallest cone margin of a stance force, in standard deviations of the feedback's input), the share of
robots whose margin is under 2 sigma next to the audit's share of deterministic violations, and the same with an actuation-noise
variance `--r` and a larger one `--r-large` (per input, in the input's units squared) entering every step through f_u.  Needs a GPU:
the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import _lib, workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402

EDGES = (-np.inf, 0.0, 1.0, 2.0, 3.0, 5.0, 10.0, np.inf)


def report(name, rec, violating):
    z = rec[:, _lib.POLICY_COV_MIN_Z]
    counts = [int(np.sum((z >= lo) & (z < hi))) for lo, hi in zip(EDGES[:-1], EDGES[1:])]
    bins = "  ".join(f"[{lo:g}, {hi:g}): {c}" for lo, hi, c in zip(EDGES[:-1], EDGES[1:], counts))
    print(f"{name}\n    cone margin in sigmas (word 0): {bins}; +inf (nothing counted): {int(np.sum(np.isposinf(z)))}; NaN: {int(np.sum(np.isnan(z)))}")
    print(f"    under 2 sigma: {np.mean(z < 2.0):6.1%} of the robots; deterministic violations (audit word 0 > 0): {violating:6.1%}; "
          f"largest trace of S {rec[:, _lib.POLICY_COV_MAX_TRACE].max():.3e}, largest input variance from feedback "
          f"{rec[:, _lib.POLICY_COV_MAX_UVAR].max():.3e}, smallest diagonal entry {rec[:, _lib.POLICY_COV_MIN_VAR].min():.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--pos", type=float, default=0.005)
    ap.add_argument("--vel", type=float, default=0.05)
    ap.add_argument("--att", type=float, default=0.01)
    ap.add_argument("--r", type=float, default=1e-4)
    ap.add_argument("--r-large", type=float, default=1e-2)
    a = ap.parse_args()
    N, B = 30, a.robots
    batch = workload.make_batch("srbd13", N, np.arange(B))
    eng = DdpEngine("srbd13", N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), consts=batch["consts"])
    eng.enable_policy(N)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(batch["params"])
    eng.policy_range_device()
    print(f"{int(eng.stats['converged'].sum())} of {B} plans converged; policy ok for {int(eng.policy()[2][:, 3].sum())}")
    violating = float(np.mean(eng.audit()[:, _lib.AUDIT_CONE] > 0.0))
    sd = np.concatenate([np.full(3, a.pos), np.full(4, a.att), np.full(3, a.vel), np.full(3, a.vel)])      # x = r | o | rdot | w
    sigma0 = np.broadcast_to(np.diag(sd ** 2), (B, eng.nx, eng.nx))
    print(f"Sigma0 = diag, standard deviations: position {a.pos} m, quaternion {a.att}, velocities {a.vel}")
    report("estimate noise alone (q = r = 0)", eng.policy_covariance(sigma0)["record"], violating)
    for r in (a.r, a.r_large):
        report(f"with actuation-noise variance r = {r:g} per input and step", eng.policy_covariance(sigma0, r=np.full((B, eng.nu), r))["record"], violating)
    eng.close()


if __name__ == "__main__":
    main()
