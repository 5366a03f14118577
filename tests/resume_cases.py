"""Resumable solves: the inputs that tests/test_resume_cpu.py (does every cut point show the kind of carried state it claims? -- C
oracle, no GPU) and tests/test_gpu_resume.py (cut + continued against uncut, byte for byte) share.

The smallest shapes at which the carry can go wrong: srbd13 at N = 10 with B = 48 instances on max_slots = 4 (12 instances per
slot: slots are reused, a carry row indexed by slot fails), srbd37 / lip30 at N = 8, B = 8 and srbd61 at N = 6, B = 4 (the
four-wavefront kernel and its one-call-site re-roll).

Kinds of carried state at a cut -- the cut points must show each of them at least once, or a wrong carry of that part of the state
would pass -- and where the workload seeds 0..47 at N = 10 show them on the C oracle:
  (a) gap > 0: multiple shooting, initial_rollout = 0, first accepted step shorter than 1.  The warm starts of the workload all
      accept a full first step under the default alpha_0 = 1 (which closes the gaps exactly), so the case is options_cases' set A
      (alpha_0 = 0.5: the gap halves per step and is never an exact zero): every unfinished instance of "A" at k = 4.
  (b) gap == 0 and theta = 1 (a full step was the last one, second_order = 1): the unfinished instances of "base" at k = 4.
  (c) mu > mu0, a bumped regularisation that has not decayed yet: NO workload seed bumps at N = 10 under the default options
      (asserted in the CPU test), so the case is the one of tests/options_cases.py that forces a bump, set E (mu0 = -1e9,
      mu_min = 3e-3: the first sweep fails, mu -> 3e-3, then a tenth per accepted step): every unfinished instance of "E" at k = 4.
  (d) converged before the cut: seeds 19, 26, 30, ... of "base" take 3 iterations, the cut is at 4.
"ir1" (single shooting) and "so0" (Gauss-Newton) are the other two settings the central test must run under.
"""
import functools

from tests import options_cases as oc, oracle_refs as refs

SHAPES = {"srbd13": (10, 48), "srbd37": (8, 8), "lip30": (8, 8), "srbd61": (6, 4)}      # model -> (N, B); seeds 0 .. B - 1
MAX_SLOTS = {"srbd13": 4, "srbd37": 2, "lip30": 2, "srbd61": 2}
OVER = {"base": {}, "ir1": dict(initial_rollout=1), "so0": dict(second_order=0), "A": dict(oc.SETS["A"]), "E": dict(oc.SETS["E"])}
CUT = {"srbd13": 4, "srbd37": 4, "lip30": 1, "srbd61": 4}      # cut + continue (lip30 is linear-quadratic: 2 iterations)
CUTS3 = {"srbd13": (2, 5), "srbd37": (2, 5), "lip30": (0, 1), "srbd61": (2, 5)}      # cut, continue, continue
TOTAL = 100
# (model, setting, waves_per_simd) of the central identity tests: cut + continued (tests/test_gpu_resume.py), a budget that never runs out
# (tests/test_gpu_deadline.py)
IDENTITY = [("srbd13", "base", 1), ("srbd13", "base", 2), ("srbd13", "ir1", 2), ("srbd13", "so0", 1), ("srbd13", "A", 2), ("srbd13", "E", 1),
            ("srbd37", "base", 1), ("srbd37", "base", 2), ("srbd37", "ir1", 2), ("srbd37", "so0", 1), ("srbd37", "E", 2),
            ("lip30", "base", 2), ("lip30", "ir1", 2), ("srbd61", "base", 1), ("srbd61", "ir1", 1)]


def options(case, **more):
    return refs.options(OVER[case], **more)


@functools.lru_cache(maxsize=None)
def batch(model):
    N, B = SHAPES[model]
    return refs.batch(model, N, range(B))


@functools.lru_cache(maxsize=None)
def oracle(model, case, max_iters=TOTAL):
    """-> (xs, us, stats [B, 8]: cport.STAT_FIELDS) of the C oracle, read-only"""
    return refs.c_oracle(model, batch(model), options(case, max_iters=max_iters))
