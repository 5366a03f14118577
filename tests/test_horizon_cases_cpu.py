"""Does the table of tests/horizon_cases.py still exercise what it claims?  No GPU: the C oracle in its two builds (`off`, `fast`) on
every case and instance.  The figures asserted here are the ones the module docstring of tests/horizon_cases.py states; an input that
has drifted shows here first."""
import numpy as np
import pytest

from oracle import cport
from tests import horizon_cases as hc, options_cases as oc

ALL = [c.name for c in hc.cases()]


def test_the_table_is_the_one_the_kernels_need():
    """every horizon at which an N-expression of the device code changes value, per kernel family"""
    assert hc.HORIZONS == {"srbd13": (1, 2, 3, 63, 64, 65, 129), "srbd37": (1, 2, 3, 5, 64, 65), "srbd61": (1, 2, 3, 65),
                           "lip30": (1, 2, 3, 5, 64, 65)}
    assert len(ALL) == 7 + 6 + 4 + 6 + 6 + 2 and set(hc.ITERS) == set(ALL)
    assert all(len(c.seeds) == 8 and set(c.seeds) <= set(range(32)) for c in hc.cases())
    assert all(c.seeds == hc.SEEDS for c in hc.cases() if c.kind != "so2")


@pytest.mark.parametrize("name", ALL)
def test_both_oracle_builds_agree_and_the_case_converges_in_the_recorded_iterations(name):
    c = hc.CASES[name]
    (xo, _, so), (xf, _, sf) = hc.oracle(name, "off"), hc.oracle(name, "fast")
    it = cport.stat(so, "iters").astype(int)
    print(f"{name}: iterations {it.tolist()} alpha {sorted(set(cport.stat(so, 'alpha').tolist()))} gap {cport.stat(so, 'gap').max():.3e} "
          f"l-inf between the builds' x {np.max(np.abs(xo - xf)):.3e}")
    for f in ("iters", "status", "converged", "alpha"):                                    # alpha: the same double
        np.testing.assert_array_equal(cport.stat(so, f), cport.stat(sf, f), err_msg=f)
    assert (cport.stat(so, "status") == 0).all() and (cport.stat(so, "converged") == 1).all()
    assert tuple(it.tolist()) == hc.ITERS[name]
    assert (cport.stat(so, "alpha") == hc.LAST_ALPHA[c.kind]).all()
    assert np.max(np.abs(xo - xf)) <= hc.BUILDS_LINF
    ro, rf = cport.stat(so, "rho"), cport.stat(sf, "rho")
    assert ((ro == 0) == (rf == 0)).all() and np.max(np.abs(ro - rf) / np.maximum(np.abs(ro), 1e-300)) <= oc.RHO_SPREAD
    if c.kind == "a05":                                                                     # the loop and the gap_tol exit did run
        assert (it >= 24).all() and (cport.stat(so, "gap") > 0).all() and (cport.stat(so, "gap") <= 1e-9).all()
    if c.kind == "so2" and c.N > 1:                                                         # the second-order term acts
        assert tuple(it.tolist()) != hc.ITERS[f"{c.model}-N{c.N}"]


@pytest.mark.parametrize("name", ALL)
def test_a_forgotten_last_knot_would_show(name):
    """the optimum at N against the optimum of the problem truncated to N - 1: further apart, in x[:N] or in cost, than 1e3 times
    what tests/test_gpu_horizons.py tolerates -- on every instance"""
    c = hc.CASES[name]
    xo, _, so = hc.oracle(name)
    xt, Jt = hc.oracle_truncated(name)
    assert xt.shape == xo[:, :c.N].shape
    dx = np.max(np.abs(xo[:, :c.N] - xt), axis=(1, 2))
    J = cport.stat(so, "cost")
    dJ = np.abs(J - Jt) / np.abs(J)
    print(f"{name}: x[:N] differs by {dx.min():.3e} .. {dx.max():.3e}, the cost by {dJ.min():.3e} .. {dJ.max():.3e} relative")
    assert ((dx >= hc.MARGIN_X) | (dJ >= hc.MARGIN_COST)).all(), (dx, dJ)


@pytest.mark.parametrize("model,N,cuts", hc.RESUME)
def test_the_resume_cuts_do_cut(model, N, cuts):
    """a cut at max_iters = k leaves status 1 on every instance that takes k steps or more (a solve of k steps notices that it has
    converged in the pass behind its last step): every cut of the table leaves something to continue, N = 1 included"""
    name = hc.case_of(model, N).name
    for k in cuts:
        st = hc.oracle(name, "off", k)[2]
        n_cut = int((cport.stat(st, "status") == 1).sum())
        print(f"{name} cut at {k}: {n_cut} unfinished")
        assert n_cut == sum(i >= k for i in hc.ITERS[name]) and n_cut >= 1


def test_largest_advance_horizons():
    from oracle import cport
    want = {"srbd13": 214, "srbd37": 109}
    for model, N in want.items():
        nx, _, npar = cport.DIMS[model]
        assert hc.largest_advance_horizon(nx, npar) == N
        assert (N + 1) * max(nx, npar) <= hc.ADVANCE_WORDS < (N + 2) * max(nx, npar)
