"""Whole solves at the edges of the horizon N: the case table that tests/test_horizon_cases_cpu.py (does every case converge, do the
two oracle builds agree on it, would a forgotten last knot show? -- C oracle, no GPU) and tests/test_gpu_horizons.py (the four kernel
families against the C oracle, and the features that index by N) share.

All device code is written against N: the one-lane-per-knot loops (`for (k = lane; k <= N; k += kWave)`, `ku = k < N ? k : N - 1`),
the sweep's and the rollout's prefetch guards (`k < N - 1`, `k > 0`, `k + 1 < N`), the candidate slots of (N+1) nx and N nu words,
the resume carry of N nx words, the policy export's `kk >= keep`, advance_kernel's last parameter row.  The other whole-solve tests
run at N in {4, 6, 8, 10, 20, 30, 60}; this table runs where those expressions change value:
  N = 1, 2, 3     both prefetch guards are false on the first knot (N = 1: N - 1 == 0; N = 2: the gain store of "the previous knot"
                  happens once); 3 is the first horizon with an interior knot
  N = 5           the four-wavefront kernels' shortest horizon with every stager at work
  N = 63, 64, 65  N + 1 knots fill one wavefront of 64 lanes exactly (63), spill one knot (64), N stage knots spill one (65)
  N = 129         a third trip of the 64-lane knot loops (srbd13)

A case = model, N, the workload seeds (B = 8), an option override on options_cases.BASE, second_order.  Kinds:
  base   BASE options, the plain build, all four models
  a05    lip30 with alpha_0 = 0.5: the problem is linear-quadratic and ends after one iteration under BASE, which says little about the
         loop; with half steps the gap halves per step and the gap_tol exit decides (options_cases set A)
  so2    srbd13 on the second_order = 2 build (the second loop of phase_derivs, `k < N`, and so2_knot)

Measured on the C oracle, builds `off` and `fast` (oracle/Makefile CONTRACT): every instance of the table ends with status 0, and the
two builds agree on iteration count, status, converged flag and last step length (to the bit) on every one of them; the largest
l-inf distance between the two builds' x is 1.2e-12 (lip30 at N = 65; 2.3e-13 on the SRBD models, srbd13 at N = 129), and rho is
zero but in the a05 cases, where the builds differ by at most 1.3e-13 relative (within options_cases.RHO_SPREAD).  ITERS holds the
iteration counts per seed, asserted by tests/test_horizon_cases_cpu.py:
  a05   N = 1: 24-25, N = 2: 25-26, N = 3: 26-27, N = 5: 27, N = 64 and 65: 30-31; every step 0.5, final gap 9e-10 <= gap_tol
  so2   N = 1: 1 each; N = 65: 10 7 20 14 18 9 5 23 (the plain build takes 10 8 20 17 24 9 5 23 there: the second-order term acts)
The so2 cases run on the seeds 0..7 like the others: the two builds agree on every one of them at N = 1 and at N = 65, so no seed
had to be replaced (SO2_SEEDS is where another choice would be written down).

Would the table show a wrong edge?  For every case the oracle's optimum at N is compared with its optimum on the same problem
truncated to N - 1 (the last stage dropped, the terminal cost at knot N - 1, parameter rows 0 .. N - 1): they differ in x[:N] by
MARGIN_X or in cost by MARGIN_COST (relative) on every instance -- 1e3 times what tests/test_gpu_horizons.py tolerates -- so a kernel
that forgets the last knot cannot pass.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import cport, ddp as oddp, models as omodels
from tests import options_cases as oc, oracle_refs as refs, parity

BASE = oc.BASE
SEEDS = tuple(range(8))
HORIZONS = {"srbd13": (1, 2, 3, 63, 64, 65, 129), "srbd37": (1, 2, 3, 5, 64, 65), "srbd61": (1, 2, 3, 65),
            "lip30": (1, 2, 3, 5, 64, 65)}
A05 = dict(alpha_0=0.5)
SO2_HORIZONS = (1, 65)
SO2_SEEDS = {1: SEEDS, 65: SEEDS}

X_TOL, COST_RTOL = parity.X_TOL, parity.COST_RTOL   # what tests/test_gpu_horizons.py tolerates (parity.assert_matches_c_oracle)
MARGIN_X, MARGIN_COST = 1e3 * X_TOL, 1e3 * COST_RTOL

Case = namedtuple("Case", "name kind model N seeds over so")


def cases():
    out = [Case(f"{m}-N{N}", "base", m, N, SEEDS, {}, 1) for m in ("srbd13", "srbd37", "srbd61", "lip30") for N in HORIZONS[m]]
    out += [Case(f"lip30-N{N}-a05", "a05", "lip30", N, SEEDS, A05, 1) for N in HORIZONS["lip30"]]
    out += [Case(f"srbd13-so2-N{N}", "so2", "srbd13", N, SO2_SEEDS[N], {}, 2) for N in SO2_HORIZONS]
    return out


CASES = {c.name: c for c in cases()}

# iterations of the C oracle per seed (both builds), measured
ITERS = {
    "srbd13-N1": (1,) * 8, "srbd13-N2": (2,) * 8, "srbd13-N3": (3, 2, 2, 3, 3, 3, 2, 3),
    "srbd13-N63": (12, 8, 19, 18, 24, 10, 5, 23), "srbd13-N64": (12, 9, 20, 19, 24, 10, 5, 24),
    "srbd13-N65": (10, 8, 20, 17, 24, 9, 5, 23), "srbd13-N129": (15, 8, 41, 33, 32, 30, 6, 29),
    "srbd37-N1": (1,) * 8, "srbd37-N2": (2,) * 8, "srbd37-N3": (3, 2, 3, 3, 3, 3, 3, 3), "srbd37-N5": (3, 3, 4, 5, 5, 3, 3, 3),
    "srbd37-N64": (4, 6, 6, 6, 5, 5, 5, 5), "srbd37-N65": (5, 6, 6, 6, 5, 5, 5, 5),
    "srbd61-N1": (1,) * 8, "srbd61-N2": (2,) * 8, "srbd61-N3": (3, 2, 3, 3, 3, 3, 2, 3), "srbd61-N65": (7, 7, 7, 8, 13, 11, 7, 8),
    "lip30-N1": (1,) * 8, "lip30-N2": (1,) * 8, "lip30-N3": (1,) * 8, "lip30-N5": (1,) * 8, "lip30-N64": (1,) * 8, "lip30-N65": (1,) * 8,
    "lip30-N1-a05": (25, 25, 25, 25, 25, 24, 25, 25), "lip30-N2-a05": (26, 26, 26, 26, 26, 25, 26, 26),
    "lip30-N3-a05": (26, 26, 27, 26, 27, 26, 26, 27), "lip30-N5-a05": (27,) * 8,
    "lip30-N64-a05": (31, 31, 31, 31, 31, 30, 31, 31), "lip30-N65-a05": (31, 31, 31, 31, 31, 30, 31, 31),
    "srbd13-so2-N1": (1,) * 8, "srbd13-so2-N65": (10, 7, 20, 14, 18, 9, 5, 23),
}
LAST_ALPHA = {"base": 1.0, "a05": 0.5, "so2": 1.0}
BUILDS_LINF = 1.2e-12      # largest l-inf distance between the two oracle builds' x over the table (lip30 at N = 65), measured

# features that index by N, at the edge horizons only (tests/test_gpu_horizons.py): model, N, cut points
RESUME = (("srbd13", 1, (1,)), ("srbd13", 65, (1, 3)), ("srbd37", 2, (1,)), ("srbd37", 65, (1, 3)), ("srbd61", 65, (1, 3)))
POLICY = (("srbd13", 1, 1), ("srbd13", 65, 65), ("srbd13", 65, 1), ("srbd37", 1, 1), ("srbd37", 65, 65), ("srbd37", 65, 1))      # model, N, knots
ADVANCE_WORDS = 4096                                # sddp_advance shifts arrays of at most (N + 1) max(nx, np) words


def options(case, **more):
    """the case's option dictionary (both sides: DdpEngine(opts=...) and oddp.DdpOptions(**...))"""
    return refs.case_options(case, second_order=case.so, **more)


@functools.lru_cache(maxsize=None)
def start(name):
    """-> dict(x0, params, xs, us, consts) of the case: the workload's warm start, read-only"""
    c = CASES[name]
    return refs.batch(c.model, c.N, c.seeds)


def consts(name):
    return refs.consts(start(name))


@functools.lru_cache(maxsize=None)
def oracle(name, variant="off", max_iters=None):
    """-> (xs [B,N+1,nx], us [B,N,nu], stats [B,8]) of the C oracle build `variant` on the case, computed once, read-only"""
    c = CASES[name]
    return refs.c_oracle(c.model, start(name), options(c) if max_iters is None else options(c, max_iters=max_iters), variant)


@functools.lru_cache(maxsize=None)
def oracle_truncated(name):
    """-> (x [B,N,nx], cost [B]) of the oracle's optimum on the case's problem cut to N - 1 stages: the last stage dropped, the
    terminal cost at knot N - 1 with that knot's parameter row.  N = 1 leaves no stage: x_0 alone and its terminal cost."""
    c, s = CASES[name], start(name)
    if c.N == 1:
        m = omodels.make_model(c.model, consts(name))
        cost = np.array([oddp.total_cost(m, s["x0"][b][None], np.zeros((0, m.nu)), s["params"][b, :1]) for b in range(len(c.seeds))])
        return s["x0"][:, None, :].copy(), cost
    xs, _, st = refs.c_oracle(c.model, s, options(c), params=s["params"][:, :c.N], xs=s["xs"][:, :c.N], us=s["us"][:, :c.N - 1])
    assert (cport.stat(st, "status") == 0).all(), (name, st)
    return xs, cport.stat(st, "cost").copy()


def case_of(model, N):
    return CASES[f"{model}-N{N}"]


def largest_advance_horizon(nx, npar):
    """the largest N sddp_advance accepts: (N + 1) max(nx, np) <= ADVANCE_WORDS"""
    return ADVANCE_WORDS // max(nx, npar) - 1
