#!/usr/bin/env python3
"""Which gain a fleet's cost is made of, before one is turned: the cost breakdown on the device.

    python examples/cost_terms.py [--robots 1024] [--barrier 6.0] [--sharpness 30.0]

`--robots` srbd13 robots are solved once (N = 30) and sddp_cost_terms gives 16 words per robot: the total, the 13 term families
(_lib.COST_TERM_NAMES) and the largest of them.  Printed is the fleet-mean share of every family in the total and how many robots have
which family as their largest, next to the plan audit's cone word (the share of plans that leave the friction cone, its worst).  The
same fleet is then solved with min_f_gain x 4 and with the friction barrier on (weight `--barrier`, sharpness `--sharpness`): the
tuning loop this call exists for, every figure computed on the device.  Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import _lib, workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402


def report(name, eng):
    terms, audit = eng.cost_terms(), eng.audit()
    total, cone = terms["total"], audit[:, _lib.AUDIT_CONE]
    print(f"{name}: mean cost {total.mean():.4e};  outside the friction cone {100.0 * np.mean(cone > 0):.1f} % of the plans, worst {cone.max():.3e}")
    for fam in _lib.COST_TERM_NAMES:
        share, first = np.mean(terms[fam] / total), int(np.sum(terms["largest"] == fam))
        if share != 0.0 or first:
            print(f"    {fam:<17s} {100.0 * share:8.3f} % of the cost (fleet mean)   largest family of {first:5d} robots")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--barrier", type=float, default=6.0)
    ap.add_argument("--sharpness", type=float, default=30.0)
    a = ap.parse_args()
    N, B = 30, a.robots
    batch = workload.make_batch("srbd13", N, np.arange(B))
    opts = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
    base = batch["consts"]
    min_f = _lib.default_consts("srbd13", **base).min_f_gain
    for name, consts in (("as configured", base), ("min_f_gain x 4", dict(base, min_f_gain=4.0 * min_f)),
                         ("friction barrier on", dict(base, friction_barrier_weight=a.barrier, friction_barrier_sharpness=a.sharpness))):
        eng = DdpEngine("srbd13", N, B, opts=opts, consts=consts)
        eng.load(batch["x0"], batch["xs"], batch["us"])
        eng.solve(batch["params"])
        report(name, eng)
        eng.close()


if __name__ == "__main__":
    main()
