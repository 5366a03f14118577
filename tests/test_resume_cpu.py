"""Resumable solves without a GPU: the fixture selection of tests/test_gpu_resume.py on the C oracle."""
import numpy as np

from oracle import cport, ddp as oddp
from tests import oracle_refs as refs, resume_cases as rc


def _trace(model, case, b):
    return refs.c_trace(model, rc.batch(model), rc.options(case), b)


def test_the_cut_points_show_every_kind_of_carried_state_on_the_c_oracle():
    """Conditions on the INPUTS of the GPU tests (no tolerance): at the committed cut rc.CUT["srbd13"] = 4 the srbd13 cases hold at least one
    instance (a) with open gaps after a first step shorter than 1, (b) with closed gaps and theta = 1, (c) with mu > mu0,
    (d) converged before the cut.  (c) comes from options_cases' set E, the case that forces a bump: no workload seed at N = 10
    bumps the regularisation under the default options, which is asserted here too.  The uncut solve is cport.solve_trace; the
    state at the cut is the C oracle's own at max_iters = k."""
    N, B = rc.SHAPES["srbd13"]
    k = rc.CUT["srbd13"]
    stat = cport.stat
    # uncut traces: iteration counts, first accepted step, the largest mu any line search ran with
    first_alpha, mu_max, iters = {}, {}, {}
    for case in ("base", "A", "E"):
        fa, mm, it = [], [], []
        for b in range(B):
            _, _, st, tr = _trace("srbd13", case, b)
            acc = [r for r in tr if r["alpha"] > 0.0]
            fa.append(acc[0]["alpha"] if acc else 0.0); mm.append(max(r["mu"] for r in tr)); it.append(int(stat(st, "iters")))
            assert int(stat(st, "iters")) == int(stat(rc.oracle("srbd13", case)[2], "iters")[b])
        first_alpha[case], mu_max[case], iters[case] = np.array(fa), np.array(mm), np.array(it)
    cut = {case: rc.oracle("srbd13", case, k)[2] for case in ("base", "A", "E")}
    unfinished = {case: stat(cut[case], "status") == 1 for case in cut}
    # (a) multiple shooting, gap > 0 at the cut, first accepted alpha < 1
    a = unfinished["A"] & (stat(cut["A"], "gap") > 0.0) & (first_alpha["A"] < 1.0)
    assert rc.options("A").get("initial_rollout", 0) == 0 and a.sum() >= 1
    assert not ((stat(cut["base"], "gap") > 0.0) & unfinished["base"]).any()      # why (a) needs set A: full first steps everywhere
    # (b) closed gaps, theta = 1: the last accepted step was a full one, second_order = 1
    bb = unfinished["base"] & (stat(cut["base"], "gap") == 0.0) & (stat(cut["base"], "alpha") == 1.0)
    assert oddp.DdpOptions(**rc.options("base")).second_order == 1 and bb.sum() >= 1
    # (c) mu > mu0 at the cut: set E; the default options never bump on these seeds
    mu0 = rc.options("E")["mu0"]
    c = unfinished["E"] & (stat(cut["E"], "mu") > max(mu0, 0.0))
    assert c.sum() >= 1
    assert (mu_max["base"] == 0.0).all()
    # (d) converged before the cut
    d = (stat(cut["base"], "status") == 0) & (iters["base"] < k)
    assert d.sum() >= 1
    # both kinds of instance in the one batch the central test cuts: finished and unfinished ones, and more instances than slots
    assert 0 < unfinished["base"].sum() < B and B > 2 * rc.MAX_SLOTS["srbd13"]
    # the three-slice cuts: something is unfinished at both, and the second is past the first
    k1, k2 = rc.CUTS3["srbd13"]
    assert k1 < k2 and (stat(rc.oracle("srbd13", "base", k2)[2], "status") == 1).any()
    print(f"cut {k}: (a) {int(a.sum())} (b) {int(bb.sum())} (c) {int(c.sum())} (d) {int(d.sum())} instances of {B}")


def test_every_model_has_something_to_continue_at_its_cut():
    """the four-wavefront models at their small shapes: the C oracle leaves an instance unfinished at the cut and at both cuts of the
    three-slice run (lip30 is linear-quadratic and done after 2 iterations: its cuts are 1 and (0, 1))"""
    for model in ("srbd37", "lip30", "srbd61"):
        for case in ("base", "ir1"):
            for k in (rc.CUT[model], *rc.CUTS3[model]):
                st = rc.oracle(model, case, k)[2]
                assert (cport.stat(st, "status") == 1).any(), (model, case, k)
            assert rc.CUTS3[model][0] < rc.CUTS3[model][1]
