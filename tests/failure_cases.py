"""The three ways a solve gives up -- status 2 (regularisation overflow), 3 (non-finite cost), 4 (line search exhausted) -- on all
four kernel families: the case table that tests/test_failure_cases_cpu.py (does every case end the way the table says, on both builds
of the C oracle and on the numpy oracle? -- no GPU) and tests/test_gpu_failure_exits.py (the kernels against the C oracle, and what
a failed instance leaves behind for its queue neighbours and for the features behind a solve) share.

A case = model, horizon, workload seeds, an option override on options_cases.BASE, the indices of the batch that fail, and how the
start is made.  The batches are the smallest that still queue (SHAPES) and INTERLEAVE healthy and failing instances: FAIL[model]
holds index 0, the last index and two adjacent ones.  healthy(name) is the all-healthy twin of a mixed batch: the same options, the
same healthy instances at the same indices, a healthy instance in place of every failing one.

Kinds (every kind on all four models unless noted):
  S2    mu0 = 2e300: every Quu pivot is >= 1e300, the first sweep fails, theta is 0 already, the bump gives 10 * 2e300 + mu_min =
        2e301 > mu_max: status 2 with iters 0, rollouts 0, alpha 0, the start returned.  Finite, accepted by validate_options,
        independent of rounding, one sweep long.  The whole batch fails.  (The policy export behind it starts at mu = 2e301, fails
        its sweep and bumps past mu_max: ok = 0, the policy case.)
  S3a   a NaN in x0[3:7] and in the same entries of the whole xs column, on the failing instances (the input of the project's first
        status-3 test)
  S3b   +inf in params[N, 0] (the commanded velocity the terminal cost tracks)
  S3c   a NaN in us[N - 1, 0]
  S3d   x0[0] = 1e160, finite: the cost overflows to inf
  S3e   S3a with initial_rollout = 1 (single shooting: the NaN spreads over the rolled-out trajectory)
        S3a..d return the start with row 0 = x0; every S3 case has iters 0, alpha 0, mu = mu0 and a non-finite cost.
  S40   line search exhausted at iteration 0: beta = 1e6 with alpha_converge_threshold = 0.5 (a ladder of two rungs; no step meets an
        Armijo fraction of 1e6) from the workload's cold start on the failing instances.  The healthy instances of the batch start
        at the optimum the C oracle reaches under BASE: their first sweep predicts ~1e-20 < cost_reduction_ths and they end with
        status 0 before any search (test_exhausted_line_search_at_an_optimum_is_status_0 covers the searching variant).
  S4m   line search exhausted AFTER accepted steps (the iterate lives in one candidate set, the failed ladder has just overwritten
        the other one, the exit copies the right one back): srbd13, alpha_converge_threshold = 0.2, seeds 8, 14, 47, 21 (2, 2, 4, 2
        iterations) beside healthy seeds; S4n: threshold 0.1, seeds 14 and 42 (6 and 5 iterations).  Seed 21 at 0.1 (10 iterations)
        is NOT used: its iterate is so ill-conditioned (candidate costs up to 1e193 J) that the numpy oracle and the C oracle
        already differ by 1.07e-8 in the final cost, beyond parity.COST_RTOL (the GPU: 1.25e-8); every mid-solve instance of the
        table agrees between the two oracles within the parity bounds (tests/test_failure_cases_cpu.py).
        srbd61: threshold 0.6 (a ladder of one rung), seeds 12, 122, 126 fail after one full step, found by searching 256 seeds of
        workload.make_batch at thresholds 0.9 .. 0.01; every rejected margin is at least 2.5 % of J.  srbd37 and lip30: that search
        (256 seeds, thresholds 0.9, 0.6, 0.5, 0.3, 0.2, 0.1, 0.01) finds no status 4 with iters > 0: they keep S40 only.

Measured on the C oracle, builds `off` and `fast` (oracle/Makefile CONTRACT): they agree on iters, status, converged and alpha (to
the bit) on EVERY instance of the table, failing and healthy; MID_ITERS holds the iterations of the mid-solve failures, asserted on the CPU.
Every failing cost is non-finite or far below 1e290 (the kernels test |J| < 1e300 where the oracle tests isfinite).
"""
import functools
from collections import namedtuple

import numpy as np

from tests import oracle_refs as refs

BASE = refs.BASE
SHAPES = {"srbd13": (30, 12), "srbd37": (20, 6), "lip30": (20, 6), "srbd61": (20, 4)}      # model -> (N, B)
MODELS = tuple(SHAPES)
FAIL = {"srbd13": (0, 4, 5, 11), "srbd37": (0, 2, 3, 5), "lip30": (0, 2, 3, 5), "srbd61": (0, 1, 3)}

MU0_S2 = 2e300
S2_OVER = dict(mu0=MU0_S2)
S40_OVER = dict(beta=1e6, alpha_converge_threshold=0.5)
S40_TRIED = 2                                        # rungs 1 and 0.5
S3_KINDS = ("S3a", "S3b", "S3c", "S3d", "S3e")
S3_OVER = {"S3a": {}, "S3b": {}, "S3c": {}, "S3d": {}, "S3e": dict(initial_rollout=1)}
HUGE_X0 = 1e160

# srbd13 mid-solve: seeds per index (failing ones at FAIL["srbd13"]) and the healthy seeds that take their place in the twin
MID = {"S4m-srbd13": dict(model="srbd13", over=dict(alpha_converge_threshold=0.2), seeds=(8, 0, 1, 2, 14, 47, 3, 4, 5, 6, 9, 21), twin=(10, 12, 13, 15)),
       "S4n-srbd13": dict(model="srbd13", over=dict(alpha_converge_threshold=0.1), seeds=(14, 0, 1, 2, 42, 14, 3, 4, 5, 6, 7, 42), twin=(9, 10, 12, 13)),
       "S4m-srbd61": dict(model="srbd61", over=dict(alpha_converge_threshold=0.6), seeds=(12, 122, 0, 126), twin=(1, 3, 4))}
MID_ITERS = {"S4m-srbd13": (2, 2, 4, 2), "S4n-srbd13": (6, 5, 6, 5), "S4m-srbd61": (1, 1, 1)}      # of the failing instances, in index order
MID_TRIED = {"S4m-srbd13": 3, "S4n-srbd13": 4, "S4m-srbd61": 1}                                      # rungs of the exhausted ladder

Case = namedtuple("Case", "name kind model N seeds over fail")


def cases():
    out = []
    for m, (N, B) in SHAPES.items():
        seeds = tuple(range(B))
        out.append(Case(f"S2-{m}", "S2", m, N, seeds, S2_OVER, tuple(range(B))))
        out += [Case(f"{k}-{m}", k, m, N, seeds, S3_OVER[k], FAIL[m]) for k in S3_KINDS]
        out.append(Case(f"S40-{m}", "S40", m, N, seeds, S40_OVER, FAIL[m]))
    out += [Case(n, "S4m", d["model"], SHAPES[d["model"]][0], d["seeds"], d["over"], FAIL[d["model"]]) for n, d in MID.items()]
    return out


CASES = {c.name: c for c in cases()}
MIXED = tuple(n for n, c in CASES.items() if c.kind != "S2")
options = refs.case_options      # (case, **more) -> the case's option dictionary, both sides


def healthy_idx(case):
    return np.array([b for b in range(len(case.seeds)) if b not in case.fail], dtype=int)


def _make(c, seeds, fail):
    """the batch of `seeds` with the case's fault put on the instances `fail`"""
    out = refs.batch(c.model, c.N, seeds)
    out.update({k: out[k].copy() for k in refs.ARRAYS})
    f = list(fail)
    optimum = functools.partial(refs.optimum, c.model, c.N, tuple(range(len(seeds))))      # the C oracle's under BASE, seeds 0..B-1
    if c.kind == "S3e":                               # single shooting: the workload's constant input does not roll out to a finite cost
        out["us"][:] = optimum()[1]                   # on every model; the optimum's inputs do
    if c.kind in ("S3a", "S3e"):
        out["x0"][f, 3:7] = np.nan
        out["xs"][f, :, 3:7] = np.nan
    elif c.kind == "S3b":
        out["params"][f, c.N, 0] = np.inf
    elif c.kind == "S3c":
        out["us"][f, c.N - 1, 0] = np.nan
    elif c.kind == "S3d":
        out["x0"][f, 0] = HUGE_X0
    elif c.kind == "S40":                             # healthy instances: at the optimum; failing ones: the cold start
        xs, us = optimum()
        h = [i for i in range(len(seeds)) if i not in f]
        out["xs"][h], out["us"][h] = xs[h], us[h]
    return refs.frozen(out)


@functools.lru_cache(maxsize=None)
def start(name):
    """-> dict(x0, params, xs, us, consts) of the case's (mixed) batch, read-only"""
    c = CASES[name]
    return _make(c, c.seeds, c.fail)


@functools.lru_cache(maxsize=None)
def healthy(name):
    """-> the all-healthy twin of the case's batch, read-only: equal to start(name) on the healthy instances"""
    c = CASES[name]
    seeds = list(c.seeds)
    if c.kind == "S4m":
        for i, b in enumerate(c.fail):
            seeds[b] = MID[name]["twin"][i]
    return _make(c, tuple(seeds), ())


def consts(name):
    return refs.consts(start(name))


@functools.lru_cache(maxsize=None)
def oracle(name, variant="off", twin=False):
    """-> (xs, us, stats [B,8]) of the C oracle build `variant` on the case's batch (twin: on its all-healthy twin), read-only"""
    c = CASES[name]
    return refs.c_oracle(c.model, healthy(name) if twin else start(name), options(c), variant)


@functools.lru_cache(maxsize=None)
def oracle_trace(name, b, variant="off"):
    """-> the line-search records (cport.solve_trace) of instance b of the case"""
    c = CASES[name]
    return tuple(refs.c_trace(c.model, start(name), options(c), b, variant)[3])


def expected_status(case):
    """-> status per instance: the kind's on the failing instances, 0 on the healthy ones"""
    st = np.zeros(len(case.seeds), dtype=int)
    st[list(case.fail)] = int(case.kind[1])
    return st
