"""The failure exits (status 2, 3, 4) on the kernel builds WITH traits -- the widened parameter rows of the "_x" builds, the two
exponential barriers, second_order = 2, and a generated user build: the sibling of tests/failure_cases.py, whose table reaches the four
plain builds only.  tests/test_failure_build_cases_cpu.py asserts on the oracles what is written here (no GPU),
tests/test_gpu_failure_exits_builds.py runs the kernels against it.

A case = kind, build, model, horizon, workload seeds, option override, failing indices.  Shapes and failing indices are
failure_cases.SHAPES and failure_cases.FAIL; constants and options are the ones the suite states already, none new:
  x             srbd13, srbd37, lip30, srbd61   variant_cases.extra_rows_problem (four linear user rows, params widened by 8)
  friction      srbd13, srbd37, srbd61          sweep_cases.FRICTION
  bound         srbd13, srbd37                  variant_cases.bounds(model)
  so2           srbd13, srbd37                  second_order = 2 at create
  so2-friction  srbd13, srbd37                  both
  user          srbd13                          the srbd13_terrain build of tests/user_terms_defs.py (ud.widen, vary = 0)
Reference: the C oracle, builds `off` and `fast`; for the user build, whose rows are non-linear, the numpy oracle wrapped with the same
rows (tests/user_terms_oracle.py: the reference of test_solves_of_a_user_build_match_the_oracle).  It has one build and no rho: its
stats carry rho = NaN, and its healthy instances are compared through parity.assert_matches_numpy_oracle.

Kinds on every build (as tests/failure_cases.py): S2 (mu0 = 2e300, the whole batch), S3a (NaN in x0[3:7] and xs[:, 3:7]), S3c (NaN in
us[N - 1, 0]), S40 (beta = 1e6, threshold 0.5; the healthy instances start at the oracle's optimum FOR THAT BUILD'S problem and options).
Kinds of one build:
  S3x  (x, user)  +inf in the widened parameter column np + 0 at node N // 2 of the failing instances; every base column stays finite
  S3v  (bound)    x0[2] and xs[:, 2] of the failing instances = upper[2] + 200: a finite input whose plain cost is finite (asserted:
                  < 1e290 with bound_barrier_weight = 0) while exp(6 x 200) overflows: only the barrier is inf
  S3f  (friction, so2-friction)  the vertical force of contact 0 at the first stance knot k >= 1 of each failing instance set to
                  -800 / sharpness = -200: row [0, 0, -1] of models.friction_cone_rows gives sharpness x a.f = 800, exp(800) = inf.
                  The oracle's start cost is inf, and finite (< 1e290) with friction_barrier_weight = 0 (asserted on the CPU).
  S4b  (bound, friction, so2-friction; srbd13)  line search exhausted AFTER accepted steps: see MID below
  Lc   (bound, friction; srbd13, srbd37)        a healthy solve with a rejected non-finite rung: see LC below

The searches (search_s4b / search_lc below, on the C oracle alone; the figures are in profiles/failure_exits/README.md):
  S4b  workload.make_batch seeds 0 .. 255 at alpha_converge_threshold 0.9, 0.6, 0.5, 0.3, 0.2, 0.1, 0.01.  A seed is used only where
       both builds of the C oracle agree on status, iters, converged and (bits) alpha and the numpy oracle agrees within the bounds of
       tests/parity.py.  What it found is in MID; a build for which MID has no entry keeps S40 only.
  Lc   the same 256 seeds, the warm start displaced as queue_order_cases displaces its starts: for `bound` NOISE_R x size x N(0, 1) on
       the CoM position of the knots 1 .. N, for `friction` NOISE_U x size x N(0, 1) on every input, size in LC_SIZES = (1, 3, 10),
       default_rng(queue_order_cases.NOISE_SEED + seed).  Wanted: status 0, converged, and at least one line search of the trace with
       a non-finite margin on a rung in front of the accepted one.  What it found is in LC.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import cport, ddp as oddp, models as omodels
from tests import failure_cases as fc, oracle_refs as refs, queue_order_cases as qc, sweep_cases, user_terms_defs as ud, variant_cases
from tests.user_terms_oracle import WithUserRows

BASE, SHAPES, FAIL = fc.BASE, fc.SHAPES, fc.FAIL
BUILDS = {"x": ("srbd13", "srbd37", "lip30", "srbd61"), "friction": ("srbd13", "srbd37", "srbd61"), "bound": ("srbd13", "srbd37"),
          "so2": ("srbd13", "srbd37"), "so2-friction": ("srbd13", "srbd37"), "user": ("srbd13",)}
SO2 = ("so2", "so2-friction")
USER_CASE = "srbd13_terrain"
OWN_KINDS = {"x": ("S3x",), "user": ("S3x",), "bound": ("S3v",), "friction": ("S3f",), "so2-friction": ("S3f",), "so2": ()}
OVERFLOW_BY, CONE_ARGUMENT = 200.0, 800.0             # S3v: past the upper bound; S3f: sharpness x a.f
THRESHOLDS = (0.9, 0.6, 0.5, 0.3, 0.2, 0.1, 0.01)     # of the S4b search (tests/failure_cases.py)
SEARCH_SEEDS = 256
LC_SIZES = (1.0, 3.0, 10.0)

# S4b, found by search_s4b: name -> seeds per index (the failing ones at FAIL[model]), the healthy seeds of the twin, the override
_S4B = dict(model="srbd13", over=dict(alpha_converge_threshold=0.2), seeds=(8, 0, 1, 2, 14, 47, 3, 4, 5, 6, 9, 21), twin=(10, 12, 13, 15))
MID = {f"S4b-{b}-srbd13": dict(_S4B, build=b) for b in ("bound", "friction", "so2-friction")}
MID_ITERS = {n: (2, 2, 4, 2) for n in MID}            # of the failing instances, in index order: the same on the three builds
# Lc, found by search_lc: name -> dict(model, build, size, seeds)
LC = {"Lc-bound-srbd13": dict(build="bound", model="srbd13", size=1.0, seeds=tuple(range(12))),
      "Lc-bound-srbd37": dict(build="bound", model="srbd37", size=3.0, seeds=tuple(range(6))),
      "Lc-friction-srbd13": dict(build="friction", model="srbd13", size=10.0, seeds=tuple(range(12))),
      "Lc-friction-srbd37": dict(build="friction", model="srbd37", size=10.0, seeds=(8, 11, 13, 17, 21, 22))}

Case = namedtuple("Case", "name kind build model N seeds over fail")


def build_options(build, over=None, **more):
    """the option dictionary of both sides on a build: BASE, second_order = 2 on the so2 builds, the override"""
    return refs.options(dict(second_order=2) if build in SO2 else {}, **(over or {}), **more)


def options(case, **more):
    return build_options(case.build, case.over, **more)


def cases():
    out = []
    for build, models in BUILDS.items():
        for m in models:
            N, B = SHAPES[m]
            seeds, tag = tuple(range(B)), f"{build}-{m}"
            out.append(Case(f"S2-{tag}", "S2", build, m, N, seeds, fc.S2_OVER, tuple(range(B))))
            out += [Case(f"{k}-{tag}", k, build, m, N, seeds, {}, FAIL[m]) for k in ("S3a", "S3c") + OWN_KINDS[build]]
            out.append(Case(f"S40-{tag}", "S40", build, m, N, seeds, fc.S40_OVER, FAIL[m]))
    out += [Case(n, "S4b", d["build"], d["model"], SHAPES[d["model"]][0], d["seeds"], d["over"], FAIL[d["model"]]) for n, d in MID.items()]
    out += [Case(n, "Lc", d["build"], d["model"], SHAPES[d["model"]][0], d["seeds"], {}, ()) for n, d in LC.items()]
    return out


CASES = {c.name: c for c in cases()}
FAILING = tuple(n for n, c in CASES.items() if c.kind != "Lc")
MIXED = tuple(n for n, c in CASES.items() if c.kind not in ("S2", "Lc"))


def healthy_idx(case):
    return np.array([b for b in range(len(case.seeds)) if b not in case.fail], dtype=int)


def expected_status(case):
    st = np.zeros(len(case.seeds), dtype=int)
    st[list(case.fail)] = int(case.kind[1]) if case.fail else 0
    return st


@functools.lru_cache(maxsize=None)
def user_spec(N):
    return ud.spec_of(ud.srbd13_terrain(N)[1])


def problem(build, model, N, seeds, **consts_over):
    """-> dict(x0, params, xs, us: the workload's batch on the build's problem, the caller's own copies; consts: the handle's
    constants; base_consts: the workload's)"""
    b = refs.batch(model, N, seeds)
    out = {k: b[k].copy() for k in refs.ARRAYS}
    consts = dict(b["consts"])
    if build == "x":
        _, out["params"], consts = variant_cases.extra_rows_problem(model, N, list(seeds))
    elif build == "user":
        spec = user_spec(N)
        out["params"] = ud.widen(b["params"], spec)
        consts["extra_rows"] = spec.extra_rows()
    elif build == "bound":
        consts.update(variant_cases.bounds(model))
    if "friction" in build:
        consts.update(sweep_cases.FRICTION)
    consts.update(consts_over)
    out.update(consts=consts, base_consts=dict(b["consts"]))
    return out


def base_columns(model):
    return cport.DIMS[model][2]


def _fz(model):
    """(input index of the vertical force of contact 0, parameter column of its contact switch)"""
    return (2, omodels.SRBD13.P_SW[0]) if model == "srbd13" else (5, 8)


def stance_knot(model, params_b):
    """the first knot k >= 1 at which contact 0 stands"""
    sw = params_b[1:-1, _fz(model)[1]]
    return 1 + int(np.flatnonzero(sw == 1.0)[0])


def _numpy_solve(build, model, s, opts, sel=None):
    """the numpy oracle on the user build -> (xs, us, stats [B, 8] in cport.STAT_FIELDS' order; rho, which it does not report: NaN)"""
    m = WithUserRows(omodels.make_model(model, omodels.RobotConsts(**s["base_consts"])), user_spec(s["us"].shape[1]))
    sel = range(len(s["x0"])) if sel is None else sel
    res = []
    with np.errstate(all="ignore"):
        for b in sel:
            res.append(oddp.solve(m, s["x0"][b], s["params"][b], s["xs"][b], s["us"][b], oddp.DdpOptions(**opts)))
    st = np.array([[r.cost, r.iters, float(r.converged), r.alpha, r.gap, r.mu, r.status, np.nan] for r in res])
    return refs.frozen((np.stack([r.xs for r in res]), np.stack([r.us for r in res]), st))


def solve_on_oracle(build, model, s, opts, variant="off", threads=4):
    """the build's reference on a start -> (xs, us, stats [B, 8]), read-only"""
    if build == "user":
        return _numpy_solve(build, model, s, opts)
    return refs.c_oracle(model, s, opts, variant, threads=threads)


@functools.lru_cache(maxsize=None)
def optimum(build, model, N, seeds):
    """-> (xs, us) the build's reference reaches from the workload's warm start under the build's options: the restart point of S40"""
    xs, us, st = solve_on_oracle(build, model, problem(build, model, N, seeds), build_options(build))
    assert (cport.stat(st, "converged") == 1).all() and (cport.stat(st, "status") == 0).all(), (build, model, st)
    return xs, us


def displaced(build, model, N, seeds, size):
    """the build's problem with the Lc displacement (module docstring) on the warm start"""
    out = problem(build, model, N, seeds)
    for b, seed in enumerate(seeds):
        rng = np.random.default_rng(qc.NOISE_SEED + int(seed))
        if build == "bound":
            out["xs"][b, 1:, 0:3] += size * qc.NOISE_R * rng.standard_normal((N, 3))
        else:
            out["us"][b] += size * qc.NOISE_U * rng.standard_normal(out["us"][b].shape)
    return out


def _make(c, seeds, fail):
    if c.kind == "Lc":
        return refs.frozen(displaced(c.build, c.model, c.N, seeds, LC[c.name]["size"]))
    out = problem(c.build, c.model, c.N, seeds)
    f, npb = list(fail), base_columns(c.model)
    if c.kind == "S3a":
        out["x0"][f, 3:7] = np.nan
        out["xs"][f, :, 3:7] = np.nan
    elif c.kind == "S3c":
        out["us"][f, c.N - 1, 0] = np.nan
    elif c.kind == "S3x":
        out["params"][f, c.N // 2, npb] = np.inf
    elif c.kind == "S3v":
        out["x0"][f, 2] = out["consts"]["upper"][2] + OVERFLOW_BY
        out["xs"][f, :, 2] = out["consts"]["upper"][2] + OVERFLOW_BY
    elif c.kind == "S3f":
        for b in f:
            out["us"][b, stance_knot(c.model, out["params"][b]), _fz(c.model)[0]] = -CONE_ARGUMENT / out["consts"]["friction_barrier_sharpness"]
    elif c.kind == "S40":
        xs, us = optimum(c.build, c.model, c.N, tuple(range(len(seeds))))
        h = [i for i in range(len(seeds)) if i not in f]
        out["xs"][h], out["us"][h] = xs[h], us[h]
    return refs.frozen(out)


@functools.lru_cache(maxsize=None)
def start(name):
    """-> dict(x0, params, xs, us, consts, base_consts) of the case's (mixed) batch, read-only"""
    c = CASES[name]
    return _make(c, c.seeds, c.fail)


@functools.lru_cache(maxsize=None)
def healthy(name):
    """-> the all-healthy twin of the case's batch: equal to start(name) on the healthy instances"""
    c = CASES[name]
    seeds = list(c.seeds)
    if c.kind == "S4b":
        for i, b in enumerate(c.fail):
            seeds[b] = MID[name]["twin"][i]
    return _make(c, tuple(seeds), ())


@functools.lru_cache(maxsize=None)
def oracle(name, variant="off", twin=False):
    """-> (xs, us, stats [B, 8]) of the reference on the case's batch (twin: on its all-healthy twin), read-only.  The user build has
    one reference: `variant` does not matter there"""
    c = CASES[name]
    return solve_on_oracle(c.build, c.model, healthy(name) if twin else start(name), options(c), variant)


def variants(case):
    return ("off",) if case.build == "user" else ("off", "fast")


@functools.lru_cache(maxsize=None)
def start_cost(name, variant="off", **consts_over):
    """-> the cost of the case's start [B] (the reference at max_iters = 0), with constants replaced"""
    c, s = CASES[name], start(name)
    s = dict(s, consts=dict(s["consts"], **consts_over))
    return cport.stat(solve_on_oracle(c.build, c.model, s, options(c, max_iters=0), variant)[2], "cost")


@functools.lru_cache(maxsize=None)
def oracle_trace(name, b, variant="off"):
    """-> the line-search records (cport.solve_trace) of instance b of the case (C oracle builds only)"""
    c = CASES[name]
    return tuple(refs.c_trace(c.model, start(name), options(c), b, variant)[3])


def rejected_non_finite(trace):
    """-> [(line search, rung)] of the rungs with a non-finite margin in front of an accepted rung"""
    out = []
    for i, r in enumerate(trace):
        if r["alpha"] > 0.0:
            out += [(i, j) for j in range(int(r["tried"]) - 1) if j < len(r["margin"]) and not np.isfinite(r["margin"][j])]
    return out


def expected_rollouts(model, trace):
    """stats.rollouts of the kernels on the oracle's ladders: one pass per 64 rungs tried, and one more where the pass did not keep the
    trajectory of the rung it accepts -- the one-wavefront kernel (srbd13) keeps the rungs 0 .. 5 of a pass, the four-wavefront kernels
    keep one rung: the one accepted last, rung 0 at the start and after a pass without a winner"""
    n, guess = 0, 0
    for r in trace:
        tried = int(r["tried"])
        passes = -(-tried // 64)
        n += passes
        if not r["alpha"] > 0.0:
            guess = 0
            continue
        win = (tried - 1) % 64
        if model == "srbd13":
            n += win >= 6
        else:
            n += win != (guess if passes == 1 else 0)
            guess = win
    return int(n)


# ---- the searches (run by hand; their findings are the tables above) ---------------------------------------------------------------
def _same_decisions(a, b):
    return np.all(a[:, [1, 2, 6]] == b[:, [1, 2, 6]], axis=1) & (a[:, 3].copy().view(np.int64) == b[:, 3].copy().view(np.int64))


def search_s4b(build, model="srbd13", threads=16):
    """-> {threshold: [(seed, iters)]} of the seeds 0 .. SEARCH_SEEDS - 1 that end with status 4 after accepted steps, on both builds of
    the C oracle with the same decisions"""
    N, seeds = SHAPES[model][0], tuple(range(SEARCH_SEEDS))
    s, found = problem(build, model, N, seeds), {}
    for th in THRESHOLDS:
        opts = build_options(build, dict(alpha_converge_threshold=th))
        a, b = (refs.c_oracle(model, s, opts, v, threads=threads)[2] for v in ("off", "fast"))
        hit = np.flatnonzero(_same_decisions(a, b) & (cport.stat(a, "status") == 4) & (cport.stat(a, "iters") > 0))
        found[th] = [(int(i), int(cport.stat(a, "iters")[i])) for i in hit]
    return found


def search_lc(build, model, threads=16):
    """-> {size: [(seed, [(line search, rung)])]}: healthy solves with a rejected non-finite rung, the same on both builds"""
    N, seeds, found = SHAPES[model][0], tuple(range(SEARCH_SEEDS)), {}
    for size in LC_SIZES:
        s = displaced(build, model, N, seeds, size)
        opts = build_options(build)
        a, b = (refs.c_oracle(model, s, opts, v, threads=threads)[2] for v in ("off", "fast"))
        found[size] = []
        for i in np.flatnonzero(_same_decisions(a, b) & (cport.stat(a, "status") == 0) & (cport.stat(a, "converged") == 1) & (cport.stat(a, "iters") > 0)):
            rungs = [rejected_non_finite(refs.c_trace(model, s, opts, int(i), v)[3]) for v in ("off", "fast")]
            if rungs[0] and rungs[0] == rungs[1]:
                found[size].append((int(i), rungs[0]))
    return found
