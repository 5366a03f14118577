"""tests/parity.py holds the tolerances of every whole-solve comparison with the C oracle; this pins them on synthetic results (no GPU):
each quantity passes at half its bound and fails at twice it, the exact ones fail on one unit / one ulp."""
import numpy as np
import pytest

from oracle import cport
from srbd_horizon_amd import _lib
from tests import options_cases as oc, parity

B, N, NX, NU = 3, 2, 4, 2


def _oracle():
    """finite, non-zero everywhere; mu of instance 2 above 1, where the relative bound is the one that binds (parity.MU_RTOL)"""
    rng = np.random.default_rng(0)
    xo, uo = rng.uniform(0.5, 2.0, (B, N + 1, NX)), rng.uniform(0.5, 2.0, (B, N, NU))
    so = np.zeros((B, len(cport.STAT_FIELDS)))
    for f, v in dict(cost=(3.5e4, 12.0, 0.7), iters=(7, 12, 3), converged=(1, 0, 1), alpha=(1.0, 0.5, 0.8 ** 3), gap=(2e-4, 3.0, 5e-9),
                     mu=(3e-8, 1e-3, 30.0), status=(0, 1, 0), rho=(40.0, 2.5e3, 0.3)).items():
        so[:, cport.STAT_FIELDS.index(f)] = v
    return xo, uo, so


def _gpu(xo, uo, so):
    st = np.zeros(B, dtype=_lib.STATS_DTYPE)
    for f in cport.STAT_FIELDS:
        st[f] = cport.stat(so, f)
    return xo.copy(), uo.copy(), st


def _check(change, **kw):
    xo, uo, so = _oracle()
    x, u, st = _gpu(xo, uo, so)
    change(x, u, st, so)
    parity.assert_matches_c_oracle(x, u, st, xo, uo, so, **kw)


def test_equal_results_pass():
    _check(lambda x, u, st, so: None)
    _check(lambda x, u, st, so: None, gap_slack=np.zeros(B), explain=lambda differ: "not asked")


def _shift_x(f):
    def change(x, u, st, so):
        x[1, 2, 3] += f * parity.X_TOL
    return change


def _shift_u(f):
    def change(x, u, st, so):
        u[2, 0, 1] -= f * parity.X_TOL
    return change


def _scale(field, rtol, b):
    return lambda f: (lambda x, u, st, so: st[field].__setitem__(b, st[field][b] * (1.0 + f * rtol)))


CHANGES = {"x": _shift_x, "u": _shift_u, "cost": _scale("cost", parity.COST_RTOL, 0), "gap": _scale("gap", parity.GAP_RTOL, 1),
           "mu": _scale("mu", parity.MU_RTOL, 2), "rho": _scale("rho", oc.RHO_RTOL, 1)}


@pytest.mark.parametrize("what", list(CHANGES))
def test_half_the_bound_passes_and_twice_the_bound_fails(what):
    change = CHANGES[what]
    _check(change(0.5))
    _check(change(-0.5))
    for f in (2.0, -2.0):
        with pytest.raises(AssertionError):
            _check(change(f))


def test_the_bounds_are_the_ones_the_gpu_tests_state():
    assert (parity.X_TOL, parity.COST_RTOL, parity.GAP_RTOL, parity.MU_RTOL) == (1e-6, 1e-9, 1e-9, 1e-12)
    assert oc.RHO_RTOL == 10.0 * oc.RHO_SPREAD == pytest.approx(1.21e-8, rel=1e-15)


@pytest.mark.parametrize("field", ["iters", "status", "converged"])
def test_one_unit_of_an_exact_quantity_fails(field):
    with pytest.raises(AssertionError):
        _check(lambda x, u, st, so: st[field].__setitem__(1, st[field][1] + 1))


def test_one_ulp_of_the_step_length_fails():
    for b, towards in ((0, 0.0), (2, 2.0)):
        with pytest.raises(AssertionError):
            _check(lambda x, u, st, so: st["alpha"].__setitem__(b, np.nextafter(st["alpha"][b], towards)))


def test_gap_slack_is_absolute_and_per_instance():
    dev = 1e-6                                                           # instance 2: gap 5e-9, so rel 1e-9 of it allows 5e-18

    def change(x, u, st, so):
        st["gap"][2] += dev
    _check(change, gap_slack=2 * dev)
    _check(change, gap_slack=np.array([0.0, 0.0, 2 * dev]))
    for slack in (0.0, 0.5 * dev, np.array([2 * dev, 2 * dev, 0.0])):
        with pytest.raises(AssertionError):
            _check(change, gap_slack=slack)


def test_differing_iterations_fail_with_the_explanation():
    def change(x, u, st, so):
        st["iters"][[0, 2]] += 1
        st["status"][1] = 3                                              # the explanation comes before any other assertion
    seen = []

    def explain(differ):
        seen.append(differ.tolist())
        return "instance 0: the explanation"
    with pytest.raises(pytest.fail.Exception, match="instance 0: the explanation"):
        _check(change, explain=explain)
    assert seen == [[0, 2]]
    with pytest.raises(AssertionError):                                  # without one: the plain comparison
        _check(change)


def test_the_numpy_oracle_comparison_of_one_instance():
    from types import SimpleNamespace
    xo, uo, so = _oracle()
    x, u, st = _gpu(xo, uo, so)
    st["gap"][0] = 0.5 * parity.GAP_CLOSED
    r = SimpleNamespace(xs=xo[0], us=uo[0], iters=7, cost=cport.stat(so, "cost")[0])
    parity.assert_matches_numpy_oracle(x[0], u[0], st[0], r)
    x[0, 1, 1] += 0.5 * parity.X_TOL
    st["cost"][0] *= 1.0 + 0.5 * parity.COST_RTOL
    parity.assert_matches_numpy_oracle(x[0], u[0], st[0], r)
    for field, value in (("iters", 8), ("cost", cport.stat(so, "cost")[0] * (1.0 + 2 * parity.COST_RTOL)), ("gap", 2 * parity.GAP_CLOSED)):
        bad = st[0].copy()
        bad[field] = value
        with pytest.raises(AssertionError):
            parity.assert_matches_numpy_oracle(x[0], u[0], bad, r)
    x[0, 1, 1] += 1.5 * parity.X_TOL
    with pytest.raises(AssertionError):
        parity.assert_matches_numpy_oracle(x[0], u[0], st[0], r)


# ---- the failed-instance comparison (status 2, 3, 4): the same bounds, NaNs allowed ------------------------------------------------------
def _failed(status=4, cost=12.0, gap=3.0):
    xo, uo, so = _oracle()
    for f, v in dict(status=status, converged=0, iters=2, alpha=0.0, cost=cost, gap=gap, mu=30.0).items():
        so[1, cport.STAT_FIELDS.index(f)] = v
    return xo, uo, so


def _check_failed(change=None, start=False, **so_kw):
    xo, uo, so = _failed(**so_kw)
    x, u, st = _gpu(xo, uo, so)
    st["rollouts"][1] = 5
    begin = None
    if start:
        begin = (xo[1, 0].copy(), xo[1].copy(), uo[1].copy())
        begin[1][0] = -1.0                                       # row 0 of the warm start is not what comes back: x0 is
    if change:
        change(x, u, st, so)
    parity.assert_failed_matches_c_oracle(x, u, st, xo, uo, so, 1, start=begin, rollouts=5)


def test_failed_instance_equal_results_pass_with_and_without_nans():
    _check_failed()
    _check_failed(start=True)
    _check_failed(status=3, cost=np.nan, gap=np.nan, start=True)
    _check_failed(status=3, cost=np.inf, gap=1e160)

    def nan_entries(x, u, st, so):
        x[1, 1, 2] = np.nan
    xo, uo, so = _failed(status=3, cost=np.nan)
    xo[1, 1, 2] = np.nan
    x, u, st = _gpu(xo, uo, so)
    parity.assert_failed_matches_c_oracle(x, u, st, xo, uo, so, 1)
    d = parity.failed_deviations(x, u, st, xo, uo, so, [1])
    assert all(np.isfinite(v) and v == 0.0 for v in d.values()), d


FAILED_SCALED = {"x": _shift_x, "u": lambda f: (lambda x, u, st, so: u.__setitem__((1, 0, 1), u[1, 0, 1] - f * parity.X_TOL)),
                 "cost": _scale("cost", parity.COST_RTOL, 1), "gap": _scale("gap", parity.GAP_RTOL, 1), "mu": _scale("mu", parity.MU_RTOL, 1)}


@pytest.mark.parametrize("what", list(FAILED_SCALED))
def test_failed_instance_half_the_bound_passes_and_twice_the_bound_fails(what):
    change = FAILED_SCALED[what]
    _check_failed(change(0.5))
    _check_failed(change(-0.5))
    for f in (2.0, -2.0):
        with pytest.raises(AssertionError):
            _check_failed(change(f))


def _set(field, b, v):
    return lambda x, u, st, so: st[field].__setitem__(b, v)


@pytest.mark.parametrize("change", [_set("status", 1, 3), _set("status", 1, 0), _set("iters", 1, 3), _set("converged", 1, 1), _set("rollouts", 1, 4),
                                    _set("alpha", 1, 5e-324), _set("cost", 1, np.nan), _set("gap", 1, np.inf)])
def test_failed_instance_exact_fields_fail_on_one_unit(change):
    with pytest.raises(AssertionError):
        _check_failed(change)


def test_failed_instance_non_finite_must_sit_where_the_oracles_does():
    with pytest.raises(AssertionError):
        _check_failed(_set("cost", 1, 12.0), status=3, cost=np.nan)
    with pytest.raises(AssertionError):
        _check_failed(_set("cost", 1, np.nan), status=3, cost=np.inf)
    with pytest.raises(AssertionError):
        _check_failed(_set("cost", 1, -np.inf), status=3, cost=np.inf)

    def one_nan(x, u, st, so):
        x[1, 2, 0] = np.nan
    with pytest.raises(AssertionError):
        _check_failed(one_nan)

    def one_bit(x, u, st, so):
        u[1, 1, 1] = np.nextafter(u[1, 1, 1], 9.0)
    with pytest.raises(AssertionError):
        _check_failed(one_bit, start=True)                       # the start comes back byte for byte
