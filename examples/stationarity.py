#!/usr/bin/env python3
"""Which robots of a fleet a second slice is worth: the stationarity certificate on the device.

    python examples/stationarity.py [--robots 1024] [--slice 6] [--worth 1e-3]

`--robots` srbd13 robots (N = 30) are solved for a first slice of `--slice` iterations, and sddp_stationarity gives 8 words per robot:
word 0 / word 3 is the reduced gradient of the returned plan relative to the size of what cancels in it.  Printed, per status of the
slice, are the quantiles of that measure.  The solves are then continued to max_iters = 100 (resumable solves) and measured again.
A cut robot (status 1) "would have been worth" the second slice if that slice brought its measure down by more than the factor
`--worth`; the last lines say how well the first slice's own record told those apart.  No threshold is built into the library.
Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import _lib, workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402

STAT, SCALE, DEFECT = (_lib.STATIONARITY_FIELDS.index(k) for k in ("stationarity", "scale", "defect"))
QUANTILES = (0.0, 0.5, 0.9, 0.99, 1.0)


def report(name, status, rel, defect):
    for s in np.unique(status):
        sel = status == s
        q = np.quantile(rel[sel], QUANTILES)
        print(f"{name:12s} status {s}: {int(sel.sum()):5d} robots, word 0 / word 3 min {q[0]:.1e}  median {q[1]:.1e}  90 % {q[2]:.1e}  99 % {q[3]:.1e}  "
              f"max {q[4]:.1e};  worst defect {defect[sel].max():.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--slice", type=int, default=6)
    ap.add_argument("--worth", type=float, default=1e-3)
    a = ap.parse_args()
    N, B = 30, a.robots
    batch = workload.make_batch("srbd13", N, np.arange(B))
    eng = DdpEngine("srbd13", N, B, opts=dict(max_iters=a.slice, alpha_converge_threshold=1e-12, beta=1e-3), consts=batch["consts"])
    eng.enable_resume()
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(batch["params"])
    status1 = eng.stats["status"].copy()
    first = eng.stationarity()
    rel1 = first[:, STAT] / first[:, SCALE]
    report(f"{a.slice} iterations", status1, rel1, first[:, DEFECT])
    eng.set_options(max_iters=100)
    eng.continue_solve()
    _, _, st = eng.fetch()
    full = eng.stationarity()
    rel2 = full[:, STAT] / full[:, SCALE]
    report("full solve", st["status"], rel2, full[:, DEFECT])
    cut = status1 == 1
    if cut.any():
        worth = cut & (rel2 < a.worth * rel1)
        print(f"cut by the first slice: {int(cut.sum())} robots; the second slice brought word 0 / word 3 down by more than {a.worth:g} x on {int(worth.sum())}")
        if worth.any() and (cut & ~worth).any():
            print(f"  their measure after the first slice: median {np.median(rel1[worth]):.1e} where it was worth it, "
                  f"{np.median(rel1[cut & ~worth]):.1e} where it was not")
        order = np.argsort(-rel1[cut])
        top = np.flatnonzero(cut)[order[:max(1, int(cut.sum()) // 4)]]
        print(f"  the quarter of the cut robots with the largest measure after the first slice holds {int(worth[top].sum())} of those {int(worth.sum())}")
    eng.close()


if __name__ == "__main__":
    main()
