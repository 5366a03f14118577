"""Does the table of tests/options_cases.py still exercise what it claims?  No GPU: the C oracle in its two builds (`off`, `fast`) on every
case and instance, and the numpy oracle on one case per model (the two oracles implement the same rule for these options).  The figures
asserted here are the ones the module docstring of tests/options_cases.py states; an input that has drifted shows here first."""
import numpy as np
import pytest

from oracle import cport, ddp as oddp, models as omodels
from tests import options_cases as oc

ALL = [c.name for c in oc.cases()]


@pytest.mark.parametrize("name", ALL)
def test_both_oracle_builds_agree_and_the_case_shows_its_facts(name):
    c = oc.CASES[name]
    so, sf = oc.oracle(name, "off")[2], oc.oracle(name, "fast")[2]
    it, alpha, status, gap, mu = (cport.stat(so, f) for f in ("iters", "alpha", "status", "gap", "mu"))
    print(f"{name}: iterations {it.astype(int).tolist()} alpha {sorted(set(alpha.tolist()))} status {sorted(set(status.astype(int).tolist()))} "
          f"gap {gap.min():.3e}..{gap.max():.3e} mu {mu.min():.3e}..{mu.max():.3e}")
    # the two builds: same iteration count, same step length to the bit, same status -- every instance
    np.testing.assert_array_equal(it, cport.stat(sf, "iters"))
    np.testing.assert_array_equal(alpha, cport.stat(sf, "alpha"))
    np.testing.assert_array_equal(status, cport.stat(sf, "status"))
    if c.kind in oc.SETS:
        assert (status == 0).all() and (cport.stat(so, "converged") == 1).all() and (it < oc.options(c)["max_iters"]).all()
        assert (alpha == oc.LAST_ALPHA[c.kind]).all()
    if c.kind in oc.ITERS:
        lo, hi = oc.ITERS[c.kind][c.model]
        assert it.min() == lo and it.max() == hi, (it.min(), it.max())
    if c.kind in "AB":
        start_gap = cport.stat(oc.oracle_start_stats(name), "gap")
        assert (gap >= start_gap * 0.5 ** it * (1 - 1e-12)).all()                   # at best halved by every step: never an exact zero
        assert (np.abs(gap / (start_gap * 0.5 ** it) - 1) <= 1e-12).sum() >= 5      # (a few instances backtrack below 0.5 on the way)
    if c.kind == "A":
        assert (gap > 0).all() and (gap <= 1e-9).all()                              # the default gap_tol decided the exit
    if c.kind == "B":
        assert (gap > 0).all() and (gap <= 1e-3).all()
        assert (gap > 1e-9).sum() >= len(c.seeds) - 2                               # ... and would not have let these through
        assert (it <= cport.stat(oc.oracle(f"A-{c.model}")[2], "iters")).all() and (it < cport.stat(oc.oracle(f"A-{c.model}")[2], "iters")).any()
    if c.kind == "D":
        assert (mu == 1e-3).all()
    if c.kind == "E":
        assert (mu > 0).all() and (mu < 3e-3).all()
        np.testing.assert_allclose(mu, 3e-3 * 0.1 ** it, rtol=1e-12)                # bumped once to mu_min, a tenth per iteration
        assert mu.max() == pytest.approx(oc.FINAL_MU_E[c.model], rel=1e-12)
    if c.kind in "FG":
        tried = oc.oracle_tried(name)
        assert tried == oc.oracle_tried(name, "fast")
        print(f"{name}: candidates per line search {[list(t) for t in tried]}")
        assert all(max(t) > 64 for t in tried)
    if c.kind == "F":
        assert [max(t) for t in tried] == [118, 160, 134] and [sum(x > 64 for x in t) for t in tried] == [6, 5, 4]
        assert it.astype(int).tolist() == [25, 31, 31] and (status == 0).all()
    if c.kind == "G":
        assert tried == ((oc.G_TRIED[c.model],) * 5,) and it[0] == 5 and status[0] == 1
        assert alpha[0] == _rung(0.8, oc.G_TRIED[c.model] - 1)
        assert (gap[0] > 0) == (c.model in oc.G_U_SHIFT)


@pytest.mark.parametrize("name,so", oc.SO_EXTRA)
def test_both_oracle_builds_agree_in_the_other_second_order_modes(name, so):
    so_, sf = oc.oracle(name, "off", so)[2], oc.oracle(name, "fast", so)[2]
    for f in ("iters", "alpha", "status"):
        np.testing.assert_array_equal(cport.stat(so_, f), cport.stat(sf, f), err_msg=f)
    assert (cport.stat(so_, "status") == 0).all() and (cport.stat(so_, "alpha") == oc.LAST_ALPHA[oc.CASES[name].kind]).all()
    rho = np.abs(cport.stat(so_, "rho") - cport.stat(sf, "rho")) / np.maximum(np.abs(cport.stat(so_, "rho")), 1e-300)
    print(f"{name} second_order={so}: iterations {cport.stat(so_, 'iters').astype(int).tolist()}, rho differs by {rho.max():.3e}")
    assert rho.max() <= oc.RHO_SPREAD


def _rung(factor, j, a=1.0):
    for _ in range(j):
        a *= factor
    return a


def test_rho_differs_between_the_builds_by_no_more_than_the_stated_spread():
    """the figure tests/test_gpu_options.py derives its tolerance for rho from (ten times RHO_SPREAD)"""
    worst = 0.0
    for name in ALL:
        ro, rf = cport.stat(oc.oracle(name, "off")[2], "rho"), cport.stat(oc.oracle(name, "fast")[2], "rho")
        assert ((ro == 0) == (rf == 0)).all()
        rel = np.max(np.abs(ro - rf) / np.maximum(np.abs(ro), 1e-300))
        worst = max(worst, rel)
    print(f"largest relative difference of rho between the two oracle builds: {worst:.3e} (RHO_SPREAD {oc.RHO_SPREAD:.3e})")
    assert worst <= oc.RHO_SPREAD


@pytest.mark.parametrize("name,b", [("D-srbd13", 0), ("C-srbd37", 0), ("B-lip30", 3), ("E-srbd61", 0)])
def test_numpy_oracle_agrees_with_the_c_oracle(name, b):
    c, s = oc.CASES[name], oc.start(name)
    m = omodels.make_model(c.model, oc.consts(name))
    r = oddp.solve(m, s["x0"][b], s["params"][b], s["xs"][b], s["us"][b], oddp.DdpOptions(**oc.options(c)))
    xo, uo, so = oc.oracle(name)
    assert r.iters == cport.stat(so, "iters")[b] and r.alpha == cport.stat(so, "alpha")[b] and r.status == cport.stat(so, "status")[b] and int(r.converged) == cport.stat(so, "converged")[b]
    assert r.mu == pytest.approx(cport.stat(so, "mu")[b], rel=1e-12) and r.gap == pytest.approx(cport.stat(so, "gap")[b], rel=1e-9)
    assert np.max(np.abs(r.xs - xo[b])) <= 1e-8 and np.max(np.abs(r.us - uo[b])) <= 1e-8
