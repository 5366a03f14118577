"""Stationarity certificate (include/sddp.h sddp_stationarity_range_device, sddp_stationarity), what needs no GPU: the numpy statement of
tests/stationarity_cases.py against central differences of the rollout cost and at the NLP fixtures' KKT points, the committed
tolerance measurements, the three declarations and the Python signatures."""
import inspect

import numpy as np
import pytest

from oracle import cport, models as omodels
from srbd_horizon_amd import _lib, workload
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.fleet import FleetQueue
from tests import abi_header, nlp_fixtures as nf, stationarity_cases as sc

EPS = np.finfo(np.float64).eps


def _rollout_cost(m, x0, u, P):
    x, J = x0, 0.0
    for k in range(u.shape[0]):
        J += m.cost(x, u[k], P[k], k)
        x = m.f(x, u[k], P[k])
    return J + m.cost(x, None, P[-1], u.shape[0])


@pytest.mark.parametrize("model", ["srbd13", "lip30"])
def test_the_reduced_gradient_is_the_gradient_of_the_rollout_cost(model):
    """Closed gaps: s_k = dJ/du_k of J(u) = the cost of the rollout from x_0, against central differences with step h = 1e-5.
    The bound, relative to word 3: truncation + rounding.  Truncation: measured at h = 1e-3, where it dominates (the difference
    quotients at h and 2 h differ by 3 x it), at most 1.09e-7 on srbd13 (4.3e-9 and 1.09e-7 on the two instances) and nothing on the
    quadratic lip30; it scales with h^2: 1.09e-11 at h = 1e-5.  Rounding: each of the two costs of a quotient carries a few eps J, so
    the quotient 2 eps J / h is allowed.  Measured |s - quotient| / word 3 at h = 1e-5: srbd13 3.7e-12 and 8.9e-12 (bound 2.7e-11 and
    2.1e-11), lip30 2.0e-11 and 1.6e-11 (bound 6.0e-11 and 5.4e-11)."""
    N, h = 4, 1e-5
    batch = workload.make_batch(model, N, [3, 4])
    m = omodels.make_model(model, omodels.RobotConsts(**batch["consts"]))
    for b in range(2):
        u = batch["us"][b] + 0.01 * np.random.default_rng(b).standard_normal(batch["us"][b].shape)
        P, x0 = batch["params"][b], batch["x0"][b]
        x = np.empty((N + 1, m.nx))
        x[0] = x0
        for k in range(N):
            x[k + 1] = m.f(x[k], u[k], P[k])
        rec, lam, s, _ = sc.model_reference(m, x, u, P)
        assert rec[sc.DEFECT] == 0.0 and rec[sc.NODES] == N
        quotient = np.zeros_like(u)
        for k in range(N):
            for i in range(m.nu):
                up, um = u.copy(), u.copy()
                up[k, i] += h
                um[k, i] -= h
                quotient[k, i] = (_rollout_cost(m, x0, up, P) - _rollout_cost(m, x0, um, P)) / (2 * h)
        bound = 1.09e-7 * (h / 1e-3) ** 2 + 2 * EPS * _rollout_cost(m, x0, u, P) / (h * rec[sc.SCALE])
        err = np.max(np.abs(quotient - s)) / rec[sc.SCALE]
        print(f"{model} instance {b}: |s - central difference| / word 3 = {err:.2e}, bound {bound:.2e}")
        assert err <= bound
        # lambda_0 likewise: dJ/dx_0, one entry
        e = np.zeros(m.nx)
        e[2] = h
        dx0 = (_rollout_cost(m, x0 + e, u, P) - _rollout_cost(m, x0 - e, u, P)) / (2 * h)
        assert abs(dx0 - lam[0, 2]) <= bound * max(rec[sc.SCALE], rec[sc.LAM_MAX], rec[sc.LAM0])


FIXTURES = nf.load_all()


@pytest.mark.parametrize("fx", FIXTURES, ids=[f["name"] for f in FIXTURES])
def test_the_nlp_optima_are_stationary(fx):
    """the fixtures are KKT points found without any DDP code: the record there, as recorded in the cases file, and below the start's"""
    opt, start = sc.fixture_records(fx)
    want = sc.FIXTURE_RECORDS[fx["name"]]
    got = (sc.relative(opt), opt[sc.DEFECT], sc.relative(start), start[sc.DEFECT])
    print(f"{fx['name']}: word 0 / word 3 {got[0]:.3e} (start {got[2]:.3e}), word 6 {got[1]:.3e} (start {got[3]:.3e})")
    # the optimum's figures are rounding: another CPU or BLAS gives other digits, within a small factor; the start's are not
    assert got[0] <= 8 * want[0] and got[1] <= 8 * want[1] and abs(got[2] - want[2]) <= 1e-3 * want[2] and abs(got[3] - want[3]) <= 1e-3 * want[3]
    assert got[0] < got[2] and got[1] < got[3]
    assert opt[sc.NODES] == fx["N"]


def test_the_committed_tolerances_are_the_measurement():
    """stationarity_cases.measure() again: the literals (rounding figures: to a factor of 2 on another CPU or BLAS, which the margin of
    64 absorbs), and where a place is decided"""
    worst, ties = sc.measure()
    committed = (sc.S_DISAGREEMENT, sc.LAMBDA_DISAGREEMENT, sc.SCALE_DISAGREEMENT, sc.F_DISAGREEMENT)
    assert all(0.0 < w <= 2.0 * c for w, c in zip(worst, committed)), (tuple(worst), committed)
    undecided = []
    for case in sc.CASES:
        model, N, B, kind = case
        batch, P, cst, xs, us, _ = sc.oracle_plans(*case)
        m = omodels.make_model(model, cst)
        for tag, x, u in (("warm start", batch["xs"], batch["us"]), ("plan", xs, us)):
            for b in range(B):
                ref = sc.model_reference(m, x[b], u[b], P[b])
                if not sc.place_decided(ref):
                    undecided.append((model, kind, tag))
                    assert sc.relative(ref[0]) <= sc.S_TOL          # ... only where all of s is below the tolerance
    assert undecided == [("lip30", "plain", "plan")] * 3 and ties.size == 52


def test_progress_on_the_c_oracles_plans():
    """what the GPU test asserts on the device, first on the C oracle alone: on the status-0 instances of the plain cases word 0 /
    word 3 at the solution is below that at the warm start -- on all 13 of them (0 that do not)"""
    total = taking_part = 0
    for case in sc.PLAIN:
        model, N, B, kind = case
        batch, P, cst, xs, us, st = sc.oracle_plans(*case)
        m = omodels.make_model(model, cst)
        for b in np.flatnonzero(cport.stat(st, "status") == 0):
            total += 1
            taking_part += sc.relative(sc.model_reference(m, xs[b], us[b], P[b])[0]) < sc.relative(sc.model_reference(m, batch["xs"][b], batch["us"][b], P[b])[0])
    assert (total, taking_part) == (13, 13)


def test_assert_result_accepts_the_reference_and_refuses_one_word_perturbed():
    case = sc.CASES[0]
    batch, P, cst, xs, us, _ = sc.oracle_plans(*case)
    m = omodels.make_model(case[0], cst)
    ref = sc.model_reference(m, xs[0], us[0], P[0])
    rec, lam, s, cand = ref
    assert sc.assert_result(rec, lam, s, ref) == (0.0, 0.0)
    assert sc.place_decided(ref)
    for word, v in ((sc.STAT, rec[sc.STAT] + 4 * sc.S_TOL * rec[sc.SCALE]), (sc.NODE, rec[sc.NODE] + 1), (sc.INPUT, (rec[sc.INPUT] + 1) % m.nu),
                    (sc.SCALE, rec[sc.SCALE] * (1 + 1e-12)), (sc.LAM0, rec[sc.LAM0] + 4 * sc.LAMBDA_TOL * rec[sc.LAM_MAX]),
                    (sc.LAM_MAX, rec[sc.LAM_MAX] * (1 + 1e-12)), (sc.DEFECT, rec[sc.DEFECT] + 1e-13), (sc.NODES, rec[sc.NODES] + 1),
                    (sc.STAT, np.nan)):
        bad = rec.copy()
        bad[word] = v
        with pytest.raises(AssertionError):
            sc.assert_result(bad, lam, s, ref)
    bad = s.copy()
    bad[2, 1] += 4 * sc.S_TOL * rec[sc.SCALE]
    with pytest.raises(AssertionError):
        sc.assert_result(rec, lam, bad, ref)
    bad = lam.copy()
    bad[3, 0] = np.nan
    with pytest.raises(AssertionError):
        sc.assert_result(rec, bad, s, ref)
    # a NaN in u at node 2: word 0 is NaN without a place, and so are the words lambda_0 .. lambda_2 reach
    u = us[0].copy()
    u[2, 0] = np.nan
    nan_ref = sc.model_reference(m, xs[0], u, P[0])
    assert np.isnan(nan_ref[0][sc.STAT]) and (nan_ref[0][sc.NODE], nan_ref[0][sc.INPUT]) == (-1, -1)
    sc.assert_result(nan_ref[0], None, None, nan_ref)
    with pytest.raises(AssertionError):
        sc.assert_result(rec, None, None, nan_ref)


def test_header_and_ctypes_agree_on_the_three_symbols():
    """the order of the parameters, which no type tells apart (the types: tests/test_abi.py, for every symbol)"""
    declared = abi_header.functions()
    assert declared["sddp_stationarity_words"] == ("int", ["sddp_handle* h", "int* words"])
    assert declared["sddp_stationarity_range_device"] == ("int", ["sddp_handle* h", "int first", "int count", "const double* d_x", "const double* d_u",
                                                                  "double* d_out", "double* d_lambda", "double* d_grad"])
    assert declared["sddp_stationarity"] == ("int", ["sddp_handle* h", "int first", "int count", "double* out"])
    structs = {"sddp_options": _lib.SddpOptions, "sddp_model_consts": _lib.SddpModelConsts, "sddp_stats": _lib.SddpStats}
    for name in ("sddp_stationarity_words", "sddp_stationarity_range_device", "sddp_stationarity"):
        res, args = _lib.SYMBOLS[name]
        ret, params = declared[name]
        assert abi_header.binds(ret, res, structs) and len(args) == len(params)
        assert all(abi_header.binds(p.rsplit(" ", 1)[0], a, structs) for p, a in zip(params, args)), name
    assert len(_lib.STATIONARITY_FIELDS) == 8 == len(set(_lib.STATIONARITY_FIELDS)) and isinstance(_lib.STATIONARITY_FIELDS, tuple)
    assert "SDDP_STATIONARITY" not in abi_header.text()                      # the word count is a function: no new constant


def test_python_signatures():
    sig = inspect.signature(DdpEngine.stationarity_device)
    assert list(sig.parameters) == ["self", "out", "first", "count", "x", "u", "lam", "grad"]
    assert [sig.parameters[k].default for k in ("first", "count", "x", "u", "lam", "grad")] == [0, None, None, None, None, None]
    sig = inspect.signature(DdpEngine.stationarity)
    assert list(sig.parameters) == ["self", "first", "count", "full"]
    assert [sig.parameters[k].default for k in ("first", "count", "full")] == [0, None, False]
    sig = inspect.signature(FleetQueue.stationarity)
    assert list(sig.parameters) == ["self", "out", "lam", "grad"] and sig.parameters["lam"].default is None
    sig = inspect.signature(FleetQueue.flush)
    assert list(sig.parameters) == ["self", "audit_out"] and sig.parameters["audit_out"].default is None
