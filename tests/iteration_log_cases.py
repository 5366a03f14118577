"""Iteration log (include/sddp.h): what tests/test_iteration_log_cpu.py (C oracle alone) and tests/test_gpu_iteration_log.py share.

Shapes, seeds, options and cut points are those of tests/resume_cases.py.  The oracle's per-line-search record is
cport.solve_trace; its first 12 words are the first 12 words of a log record.

Settings.  The five of resume_cases ("base", "A", "E", "so0", "ir1") and two more, because two kinds of record that the log must
show do not occur under those five:
  "T"  base with alpha_converge_threshold = 0.9: the ladder holds the full step alone, so a search with theta = 1 that rejects it
       fails and is redone with theta = 0 -- the theta-retry PAIR of records (srbd13 seeds 8, 23 and 44).  Under the five settings
       no srbd13 seed of 0..999 at N = 10 (and none of 0..255 at N = 30) shows a failed search with theta = 1 on the C oracle:
       a ladder down to 1e-12 fails only where the second-order direction is no descent direction at all.
  "Z"  ir1 started from the optimum the C oracle reaches under "base" (a restart, like options_cases' case G): the first sweep
       predicts no decrease, the solve ends at the convergence test before any line search and writes NO record.
Instances on which the two CPU builds of the oracle (-ffp-contract=off / fast) disagree in the number of records or in any accepted
step length are left out of the GPU-against-oracle comparison (excluded()); tests/test_iteration_log_cpu.py bounds how many that
may be.  srbd13 "ir1" on seeds 0..47 has six such instances (4, 8, 14, 29, 34, 44: single shooting at N = 10 runs some of them to
max_iters along a path that one rounding decides), so its oracle comparison runs on IR1_SEEDS instead (the tests that compare GPU
results with GPU results run "ir1" on seeds 0..47 like every other setting).
"""
import functools

import numpy as np

from oracle import cport
from tests import options_cases as oc, oracle_refs as refs, parity, resume_cases as rc

SETTINGS = ("base", "A", "E", "so0", "ir1", "T", "Z")
EXTRA = {"T": dict(alpha_converge_threshold=0.9), "Z": dict(initial_rollout=1)}
# srbd13 "ir1" against the oracle: the first 48 seeds on which the oracle's two builds take the same steps AND agree in every accepted
# cost to a tenth of the cost's bound (single shooting at N = 10 is ill-conditioned: on seeds 3, 9, 13, 23, 24, 33, 39 the builds
# take the same steps and still differ by 1e-8 .. 1e-5 in J, on 4, 8, 14, 29, 34, 44 they take other steps)
IR1_SEEDS = (0, 1, 2, 5, 6, 7, 10, 11, 12, 15, 16, 17, 18, 19, 20, 21, 22, 25, 26, 27, 28, 30, 31, 32, 35, 36, 37, 38, 40, 41, 42, 43, 45, 46,
             47, 50, 51, 52, 55, 56, 57, 58, 60, 61, 62, 63, 65, 66)
# Bounds of the GPU-against-oracle comparison for the three fields tests/test_gpu_options.py has no bound of its own for: expected, A1
# and B2 are models of a cost change, sums over the knots that cancel to (next to) nothing near the optimum; they enter the step
# test beside differences of J.  So they are held to the cost's own bound as an absolute one, COST_RTOL |J| (test_gpu_options: cost rel
# 1e-9), plus the relative bound of rho = 2 max(A1, A1 + B2) / gap, the one quantity made of them that test_gpu_options does bound
# (RHO_RTOL = ten times the spread of the oracle's two builds).  tests/test_iteration_log_cpu.py asserts that the oracle's two builds
# differ by at most a tenth of this bound.
COST_RTOL = parity.COST_RTOL
MODEL_RTOL = oc.RHO_RTOL
ROWS = 128                                   # log rows per instance in the GPU tests: more than any solve here needs (max_iters = 100)
F = {n: i for i, n in enumerate(("J", "A1", "B2", "rho", "gap", "expected", "alpha", "J_accepted", "theta", "mu", "tried", "slack",
                                 "iters", "rollouts", "mu_bumps", "reserved"))}


def options(case, **more):
    return dict(rc.options(case if case in rc.OVER else "base"), **EXTRA.get(case, {}), **more)


@functools.lru_cache(maxsize=None)
def batch(model, case="base"):
    """the start of (model, setting), read-only: resume_cases' batch; srbd13 "ir1" on IR1_SEEDS; "Z" restarted from the oracle's optimum"""
    N, B = rc.SHAPES[model]
    if model == "srbd13" and case == "ir1":
        assert len(IR1_SEEDS) == B
        return refs.batch(model, N, IR1_SEEDS)
    if case == "Z":
        xs, us = refs.optimum(model, N, tuple(range(B)))
        return dict(rc.batch(model), xs=xs, us=us)
    return rc.batch(model)


@functools.lru_cache(maxsize=None)
def traces(model, case, variant="off"):
    """-> (list over the instances of [n, 12] arrays: the oracle's records, stats [B, 8]) of the uncut solve"""
    s = batch(model, case)
    recs, stats = [], []
    for b in range(len(s["x0"])):
        _, _, st, tr = refs.c_trace(model, s, options(case), b, variant)
        recs.append(np.array([[r[k] for k in cport.TRACE_FIELDS] for r in tr]).reshape(len(tr), 12))
        stats.append(st)
    return refs.frozen(recs), np.array(stats)


@functools.lru_cache(maxsize=None)
def excluded(model, case):
    """the instances on which the oracle's two builds disagree in record count or in an accepted step length -- or take the same steps
    and differ in an accepted cost by more than a tenth of the cost's bound: no reference for a comparison at that bound either"""
    a, c = traces(model, case, "off")[0], traces(model, case, "fast")[0]

    def unstable(p, q):
        if len(p) != len(q) or (p[:, F["alpha"]] != q[:, F["alpha"]]).any():
            return True
        return bool((np.abs(p[:, F["J_accepted"]] - q[:, F["J_accepted"]]) > 0.1 * COST_RTOL * np.abs(p[:, F["J_accepted"]])).any())
    return tuple(b for b in range(len(a)) if unstable(a[b], c[b]))
