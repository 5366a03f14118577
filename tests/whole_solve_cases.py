"""Whole solves to convergence against the C oracle at the shapes of the older model tests: the inputs that
tests/test_whole_solve_cases_cpu.py (do the oracle's two builds agree on every row? -- no GPU) and the GPU tests of srbd61, the point
feet, the user rows and configs[4] (gpu_support.whole_solve) share.

A case = model, N, workload seeds, the noise on the warm start (noise x N(0, 1) from default_rng(noise_seed) on every state, x_0
kept: every node's defect open), what it changes in the workload's constants, its option override on BASE.  Kinds:
  srbd61      the eight-point robot: N = 20 on the handle's default constants, the two converged shapes (N = 60 with open defects;
              N = 20 over 40 seeds), the extreme horizons N = 1, 2, 70
  pointfeet   srbd37 / lip30 without the relative-velocity rows (number_of_legs = 4 x contact_model = 1)
  rows        the four user rows of variant_cases.extra_rows_problem on every model; srbd13 runs on both waves_per_simd builds
  config5     BASELINE configs[4] at its real size: srbd37, N = 60, 12 seeds, open defects
Measured on the C oracle, builds `off` and `fast` (oracle/Makefile CONTRACT): every instance ends converged with status 0 and
rho = gap = 0; the builds agree on iters, status, converged and alpha (to the bit) on every instance; their x differ by at most
1.7e-9 (rows-srbd13-N30, whose longest solve takes 65 iterations; 3.5e-13 on every other row).  No seed had to be replaced.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import oracle_refs as refs, variant_cases

Case = namedtuple("Case", "name kind model N seeds noise noise_seed consts over")
POINT_FEET, NOISE = dict(relative_velocity_constraints=0), 1e-3


def _case(name, kind, model, N, first, B, noise=0.0, noise_seed=None, consts=None):
    return Case(name, kind, model, N, tuple(range(first, first + B)), noise, noise_seed, consts or {}, {})


def cases():
    out = [_case("srbd61-default", "srbd61", "srbd61", 20, 0, 6), _case("srbd61-N60", "srbd61", "srbd61", 60, 20, 8, NOISE, 9),
           _case("srbd61-N20", "srbd61", "srbd61", 20, 20, 40)]
    out += [_case(f"srbd61-N{N}", "srbd61", "srbd61", N, 0, B) for N, B in ((1, 2), (2, 3), (70, 1))]
    out += [_case(f"pointfeet-{m}-N{N}", "pointfeet", m, N, 3, B, consts=POINT_FEET) for m, N, B in (("srbd37", 20, 24), ("srbd37", 60, 6), ("lip30", 20, 16))]
    out += [_case(f"rows-{m}-N{N}", "rows", m, N, 1, B) for m, N, B in (("srbd13", 30, 48), ("srbd37", 20, 16), ("srbd37", 60, 4), ("lip30", 20, 12), ("srbd61", 20, 6))]
    out.append(_case("config5-srbd37-N60", "config5", "srbd37", 60, 20, 12, NOISE, 9))
    return out


CASES = {c.name: c for c in cases()}
# iterations of the C oracle (both builds), smallest and largest over the seeds, measured
ITERS = {"srbd61-default": (5, 8), "srbd61-N60": (7, 12), "srbd61-N20": (5, 11), "srbd61-N1": (1, 1), "srbd61-N2": (2, 2), "srbd61-N70": (5, 5),
         "pointfeet-srbd37-N20": (4, 21), "pointfeet-srbd37-N60": (12, 23), "pointfeet-lip30-N20": (1, 1),
         "rows-srbd13-N30": (5, 65), "rows-srbd37-N20": (4, 8), "rows-srbd37-N60": (5, 6), "rows-lip30-N20": (1, 1), "rows-srbd61-N20": (5, 7),
         "config5-srbd37-N60": (5, 6)}
options = refs.case_options      # (case, **more) -> the case's option dictionary, both sides


@functools.lru_cache(maxsize=None)
def start(name):
    """-> dict(x0, params, xs, us, consts) of the case, read-only; "rows": plain = the plain model's (params, consts) on the same batch"""
    c = CASES[name]
    out = refs.batch(c.model, c.N, c.seeds)
    if c.kind == "rows":
        _, P, consts = variant_cases.extra_rows_problem(c.model, c.N, list(c.seeds))
        out.update(params=P, consts=consts, plain=(out["params"], out["consts"]))
    out["consts"] = dict(out["consts"], **c.consts)
    if c.noise:
        xs = out["xs"] + c.noise * np.random.default_rng(c.noise_seed).standard_normal(out["xs"].shape)
        xs[:, 0] = out["x0"]
        out["xs"] = xs
    return refs.frozen(out)


@functools.lru_cache(maxsize=None)
def oracle(name, variant="off"):
    """-> (xs, us, stats [B, 8]: cport.STAT_FIELDS) of the C oracle build `variant` on the case, computed once, read-only"""
    c = CASES[name]
    return refs.c_oracle(c.model, start(name), options(c), variant)
