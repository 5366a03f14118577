"""The solver options away from their defaults: the case table that tests/test_options_cases_cpu.py (does every case still exercise
what it claims? -- C oracle, both builds) and tests/test_gpu_options.py (the four kernels against the C oracle) share.

Every GPU test of the project builds its options from BASE; alpha_0, line_search_decrease_factor, gap_tol, mu_min and a positive mu0
never left their defaults there, and so some branches of the four pieces of device code that restate the iteration rule (solve_instance,
its four-wavefront twin, the two policy kernels) never ran: the second trip of the 64-lane line-search ladder, theta = (second_order &&
alpha == alpha_0) with alpha_0 != 1, gap_tol as the deciding exit condition, has_gap of the policy kernels with 0 < gap <= gap_tol,
mu_min in the bump and mu0 > 0 as the floor of the decay.

A case = model, horizon, workload seeds, an option override on top of BASE, how the start is made ("warm": the multiple-shooting warm
start of workload.make_batch; "restart": the optimum the C oracle reaches with BASE from that warm start, case G) and the facts the oracle must
show for it.  The figures below were measured on the C oracle, builds `off` and `fast` (oracle/Makefile CONTRACT), which agree on
iteration count, last step length (to the bit) and status on EVERY instance of the table; a seed on which they do not has no place here.

Sets A..E, all four models, seeds 0..11, warm start (iterations: range over the 12 seeds):
  A  alpha_0 = 0.5                         last step 0.5 (every step, but for srbd13's backtracking), status 0; srbd13 32-53, srbd37 30-33, lip30 28-29, srbd61 30-33
  B  alpha_0 = 0.5, gap_tol = 1e-3         status 0; srbd13 24-53, srbd37 23-24, lip30 18-19, srbd61 22-23; 0 < gap <= gap_tol
  C  alpha_0 = 0.8, factor = 0.7           last step 0.8; srbd13 14-38, srbd37 13-14, lip30 12-13, srbd61 13-14
  D  mu0 = 1e-3                            final mu exactly 1e-3, last step 1; srbd13 5-33, srbd37 4-6, lip30 2, srbd61 5-10
  E  mu0 = -1e9, mu_min = 3e-3             first sweep fails, mu -> 3e-3, then tenths: final mu 3e-8 (srbd13, srbd61), 3e-7 (srbd37),
                                           3e-5 (lip30) on the shortest solve of the 12, 3e-3 x 10^-iters on every one; last step 1
Case F (ladders longer than one wavefront on the one-wavefront kernel): srbd13, factor = 0.97, seeds 2, 8, 18; the longest line search
  tries 118, 160, 134 step lengths, 6, 5, 4 searches of each solve go past 64 candidates, the solves take 25, 31, 31 iterations.
  (Seeds 3, 7, 14, 23, 29, 42 have ladders as long, but the two oracle builds already disagree on them: not used.)
Case G (the same branch on the four-wavefront kernels, whose normal starts never backtrack beyond 3 candidates; srbd61's kOneCallSite
  re-roll is code of its own): seed 7, restart from the optimum the C oracle reaches under BASE, with an Armijo fraction beta so large
  that nothing but a step of ~1e-9 passes the test (through its 1e-13 (|J| + rho gap) slack term): accepted <=> beta a |A1| <= slack.
  THE RECIPE AS FIRST PROPOSED (factor 0.9, beta 1e6, max_iters 5, cost_reduction_ths 1e-12) IS DECIDED BY ROUNDING and is not used:
  its solves end through |dJ| < 1e-12 at |J| = 4.5e4 (srbd37; one ulp is 7e-12, so the exit asks whether J_new == J to the bit), and
  the rungs of a 0.9 ladder are 10 % apart where the noise of dphi is ~1 % of the slack.  Measured: srbd37 `off` 4 steps after
  124, 124, 123, 123 candidates, `fast` 3 steps after 124, 124, 124; srbd13 `off` 1 step after 111, `fast` 5 steps; srbd61 both 5 steps
  after 192, status 1 against 0; and 1e-12 perturbations of the start give 1 to 5 steps.  Two builds that disagree: no place in the table.
  USED INSTEAD, the same idea made robust: factor 0.8 (rungs 20 % apart), cost_reduction_ths 0 (neither cost exit can fire: every solve
  takes its max_iters = 5 steps, status 1) and a beta per model that puts the threshold slack / (beta |A1|) mid-way between two rungs:
    srbd13  beta 7e9    five steps, each accepted after 93 candidates (lane 28 of the second trip), alpha 0.8^92 = 1.214e-9
    srbd37  beta 1e9    five steps after 90 candidates each, alpha 0.8^89 = 2.371e-9
    srbd61  beta 1.8e6  five steps after 94 candidates each, alpha 0.8^93 = 9.713e-10
    lip30   beta 1e4    the problem is linear-quadratic: the BASE solve ends at the exact minimiser, the restart's sweep predicts
                        1e-22 and there is nothing to search.  Its start is therefore the optimum with every input raised by 1e-6,
                        which also opens the gaps (4.5e-5): five steps after 112 candidates each, alpha 0.8^111 = 1.750e-11, with
                        gap > 0 (the merit-function terms take part)
  Each of these gives the same iteration count, status and candidate counts on both builds, from either build's optimum, and with
  beta scaled by 0.95 and 1.05 (12 runs per model): the decision is 5 % away from a rung, the rounding noise is ~1 %.

rho: the two builds differ by at most 1.21e-9 relative over the whole table (C-srbd13; A, B, C elsewhere 1e-13..5e-12; rho = 0 in
D..G but lip30's G, where they agree to the bit).  RHO_SPREAD is that figure; the GPU may differ from the oracle by RHO_RTOL, ten times it.
"""
import functools
from collections import namedtuple

from oracle import cport
from tests import oracle_refs as refs

BASE = refs.BASE
HORIZON = {"srbd13": 30, "srbd37": 20, "lip30": 20, "srbd61": 20}
MODELS = tuple(HORIZON)

SETS = {"A": dict(alpha_0=0.5),
        "B": dict(alpha_0=0.5, gap_tol=1e-3),
        "C": dict(alpha_0=0.8, line_search_decrease_factor=0.7),
        "D": dict(mu0=1e-3),
        "E": dict(mu0=-1e9, mu_min=3e-3)}
SET_SEEDS = tuple(range(12))
LAST_ALPHA = {"A": 0.5, "B": 0.5, "C": 0.8, "D": 1.0, "E": 1.0}
ITERS = {"A": {"srbd13": (32, 53), "srbd37": (30, 33), "lip30": (28, 29), "srbd61": (30, 33)},      # measured ranges (docstring)
         "B": {"srbd13": (24, 53), "srbd37": (23, 24), "lip30": (18, 19), "srbd61": (22, 23)},
         "C": {"srbd13": (14, 38), "srbd37": (13, 14), "lip30": (12, 13), "srbd61": (13, 14)},
         "D": {"srbd13": (5, 33), "srbd37": (4, 6), "lip30": (2, 2), "srbd61": (5, 10)}}
FINAL_MU_E = {"srbd13": 3e-8, "srbd37": 3e-7, "lip30": 3e-5, "srbd61": 3e-8}      # of the shortest solve; 3e-3 x 10^-iters for every one

F_OVER = dict(line_search_decrease_factor=0.97)
F_SEEDS = (2, 8, 18)
G_OVER = dict(line_search_decrease_factor=0.8, max_iters=5, cost_reduction_ths=0.0)
G_BETA = {"srbd13": 7e9, "srbd37": 1e9, "lip30": 1e4, "srbd61": 1.8e6}
G_U_SHIFT = {"lip30": 1e-6}                        # added to every input of the optimum (docstring)
G_TRIED = {"srbd13": 93, "srbd37": 90, "lip30": 112, "srbd61": 94}
G_SEED = 7
RHO_SPREAD = 1.21e-9                               # largest relative difference of rho between the two oracle builds (docstring)
RHO_RTOL = 10.0 * RHO_SPREAD                       # GPU against the oracle (tests/parity.py)

# sets A..E beside the default second_order = 1: Gauss-Newton (0) on a four-wavefront model, full second order (2) on the one-wavefront one
SO_EXTRA = tuple((f"{k}-srbd37", 0) for k in SETS) + tuple((f"{k}-srbd13", 2) for k in SETS)

Case = namedtuple("Case", "name kind model N seeds over start")


def cases():
    out = [Case(f"{k}-{m}", k, m, HORIZON[m], SET_SEEDS, SETS[k], "warm") for k in SETS for m in MODELS]
    out.append(Case("F-srbd13", "F", "srbd13", HORIZON["srbd13"], F_SEEDS, F_OVER, "warm"))
    out += [Case(f"G-{m}", "G", m, HORIZON[m], (G_SEED,), dict(G_OVER, beta=G_BETA[m]), "restart") for m in MODELS]
    return out


CASES = {c.name: c for c in cases()}
options = refs.case_options      # (case, **more) -> the case's option dictionary, both sides


@functools.lru_cache(maxsize=None)
def start(name):
    """-> dict(x0, params, xs, us, consts) of the case, read-only; "restart": xs, us = the C oracle's (`off`) optimum under BASE"""
    c = CASES[name]
    out = refs.batch(c.model, c.N, c.seeds)
    if c.start == "restart":
        xs, us = refs.optimum(c.model, c.N, c.seeds)
        out["xs"], out["us"] = xs, us + G_U_SHIFT.get(c.model, 0.0)
    return refs.frozen(out)


def consts(name):
    return refs.consts(start(name))


@functools.lru_cache(maxsize=None)
def oracle(name, variant="off", second_order=1):
    """-> (xs [B,N+1,nx], us [B,N,nu], stats [B,8]) of the C oracle build `variant` on the case, computed once, read-only"""
    c = CASES[name]
    return refs.c_oracle(c.model, start(name), options(c, second_order=second_order), variant)


@functools.lru_cache(maxsize=None)
def oracle_start_stats(name):
    """-> stats [B,8] of the start itself (max_iters = 0): its cost and defect norm"""
    c = CASES[name]
    return refs.c_oracle(c.model, start(name), options(c, max_iters=0))[2]


@functools.lru_cache(maxsize=None)
def oracle_tried(name, variant="off"):
    """-> per instance the tuple of `tried` (candidates rolled out) of every line search of the solve, from cport.solve_trace"""
    c = CASES[name]
    out = []
    for b in range(len(c.seeds)):
        _, _, st, tr = refs.c_trace(c.model, start(name), options(c), b, variant)
        assert cport.stat(st, "iters") == cport.stat(oracle(name, variant)[2], "iters")[b]
        out.append(tuple(int(r["tried"]) for r in tr))
    return tuple(out)
