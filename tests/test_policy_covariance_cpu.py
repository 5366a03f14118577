"""Plan uncertainty (include/sddp.h sddp_policy_covariance_device), what needs no GPU: the rule of tests/policy_covariance_cases.py
on the oracle alone -- symmetry and positive semi-definiteness, the transition-matrix identity on the linear model, the sigma points
of the linearised closed loop -- and the binding of the two symbols."""
import functools
import inspect

import numpy as np

from oracle import ddp as oddp, models as omodels
from srbd_horizon_amd import _lib, workload
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.fleet import FleetQueue
from tests import abi_header, policy_cases as pc, policy_covariance_cases as cvc, policy_rollout_cases as prc
from tests.oracle_refs import frozen

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
M = 4
ML = 0.5 / np.sqrt(2.0)


def test_header_and_ctypes_agree_on_the_two_symbols():
    declared = abi_header.functions()
    assert declared["sddp_policy_covariance_words"][1] == ["sddp_handle* h", "int* words"]
    assert declared["sddp_policy_covariance_device"][1] == [
        "sddp_handle* h", "int first", "int count", "int start", "int steps", "const double* d_sigma0", "const double* d_q", "const double* d_r",
        "double friction_coefficient", "double* d_out", "double* d_cov", "double* d_ucov_diag"]
    for name in ("sddp_policy_covariance_words", "sddp_policy_covariance_device"):
        assert len(_lib.SYMBOLS[name][1]) == len(declared[name][1]), name
    assert _lib.POLICY_COV_WORDS == 16 and abi_header.defines()["SDDP_ABI_VERSION"] == 9
    names = [n for n in vars(_lib) if n.startswith("POLICY_COV_") and n != "POLICY_COV_WORDS"]
    assert sorted(getattr(_lib, n) for n in names) == list(range(15))
    assert (_lib.POLICY_COV_MIN_Z, _lib.POLICY_COV_TRACE, _lib.POLICY_COV_MAX_UVAR, _lib.POLICY_COV_MIN_VAR, _lib.POLICY_COV_OK) == (0, 6, 9, 12, 14)


def test_engine_and_fleet_methods_and_defaults():
    sig = inspect.signature(DdpEngine.policy_covariance_device)
    assert list(sig.parameters) == ["self", "sigma0", "out", "q", "r", "cov", "ucov_diag", "first", "count", "start", "steps", "friction"]
    assert [sig.parameters[p].default for p in ("q", "r", "cov", "ucov_diag", "first", "count", "start", "steps", "friction")] == \
        [None, None, None, None, 0, None, 0, None, 0.0]
    sig = inspect.signature(DdpEngine.policy_covariance)
    assert list(sig.parameters) == ["self", "sigma0", "q", "r", "first", "count", "start", "steps", "friction"]
    assert callable(FleetQueue.policy_covariance)


@functools.lru_cache(maxsize=None)
def _plan():
    """a short oracle solve of srbd13 (N = 6) and its policy by tests/policy_cases.py: computed once, read-only"""
    b = workload.make_batch("srbd13", 6, [3])
    m = omodels.make_model("srbd13", omodels.RobotConsts(**b["consts"]))
    opt = oddp.DdpOptions(**OPTS)
    P = b["params"][0]
    r = oddp.solve(m, b["x0"][0], P, b["xs"][0], b["us"][0], opt)
    _, K, info = pc.oracle_policy(m, r.xs, r.us, P, dict(gap=r.gap, mu=r.mu, alpha=r.alpha, status=r.status), opt, M)
    assert info[3] == 1.0
    return (m, *frozen((r.xs, r.us, P, K)))


def test_the_covariances_stay_symmetric_and_positive_semi_definite():
    m, xs, us, P, K = _plan()
    rng = np.random.default_rng(0)
    q, r = 1e-6 * rng.random(m.nx), 1e-4 * rng.random(m.nu)
    for ok in (1, 0):
        ref = cvc.covariance_reference(m, xs, us, P, K, ok, cvc.general_s0(m.nx, 1), q, r, 0, M, ML)
        for S in ref["cov"]:
            assert np.max(np.abs(S - S.T)) <= 1e-15 * np.max(np.abs(S))
            assert np.min(np.linalg.eigvalsh(0.5 * (S + S.T))) >= -1e-15 * np.max(np.abs(S))
        assert ref["record"][12] > 0.0 and ref["record"][13] == M and ref["record"][14] == ok
        assert (ref["record"][0] == np.inf) == (ok == 0) and np.all(ref["ucov_diag"] >= 0.0) and (ref["ucov"].any() == bool(ok))
    # and the record shadows itself
    ref = cvc.covariance_reference(m, xs, us, P, K, 1, cvc.general_s0(m.nx, 1), q, r, 1, M - 1, ML)
    assert cvc.assert_one_step(m, xs, us, P, K, 1, q, r, 1, ref["cov"]) == 0.0
    np.testing.assert_array_equal(cvc.assert_record(m, us, P, K, 1, 1, ML, ref["record"], ref["cov"], ref["ucov_diag"]), ref["record"])


def test_ok_zero_never_reads_the_gains():
    m, xs, us, P, K = _plan()
    S0 = cvc.general_s0(m.nx, 2)
    a = cvc.covariance_reference(m, xs, us, P, np.full_like(K, np.nan), 0, S0, None, None, 0, M, ML)
    b = cvc.covariance_reference(m, xs, us, P, K, 0, S0, None, None, 0, M, ML)
    np.testing.assert_array_equal(a["cov"], b["cov"])
    np.testing.assert_array_equal(a["record"], b["record"])
    assert not a["ucov"].any() and a["record"][0] == np.inf and tuple(a["record"][1:4]) == (-1, -1, -1)


def test_only_the_lower_triangle_of_sigma0_counts():
    m, xs, us, P, K = _plan()
    S0 = cvc.general_s0(m.nx, 3)
    junk = S0 + np.triu(np.ones_like(S0), 1)
    np.testing.assert_array_equal(cvc.covariance_reference(m, xs, us, P, K, 1, junk, None, None, 0, M, ML)["cov"],
                                  cvc.covariance_reference(m, xs, us, P, K, 1, S0, None, None, 0, M, ML)["cov"])


LIP_N, LIP_B = 6, 3


@functools.lru_cache(maxsize=None)
def lip_plans():
    """-> (model, [(xs, us, P, K) per instance]) of the lip30 problem by the oracle: computed once, read-only"""
    from tests import plan_audit_cases as pac
    batch, P, consts, _ = pac.problem("lip30", LIP_N, LIP_B, "plain")
    m = omodels.make_model("lip30", omodels.RobotConsts(**consts))
    opt = oddp.DdpOptions(**pac.OPTS)
    plans = []
    for b in range(LIP_B):
        r = oddp.solve(m, batch["x0"][b], P[b], batch["xs"][b], batch["us"][b], opt)
        _, K, info = pc.oracle_policy(m, r.xs, r.us, P[b], dict(gap=r.gap, mu=r.mu, alpha=r.alpha, status=r.status), opt, LIP_N)
        assert info[3] == 1.0
        plans.append(frozen((r.xs, r.us, P[b], K)))
    return m, plans


def test_on_the_linear_model_the_recursion_is_the_transition_matrix():
    m, plans = lip_plans()
    worst = 0.0
    for xs, us, P, K in plans:
        Phi = cvc.transition_matrix(lambda x0: prc.rollout_reference(m, xs, us, P, K, 1, x0, 0, LIP_N)[0][LIP_N], xs[0])
        for seed in range(5):
            S0 = cvc.general_s0(m.nx, 100 + seed)
            got = cvc.covariance_reference(m, xs, us, P, K, 1, S0, None, None, 0, LIP_N, ML)
            worst = max(worst, cvc.identity_error(got["cov"][LIP_N], Phi, S0))
            assert got["record"][0] == np.inf and not got["cone"]                  # no force inputs: no cone triple
    print(f"lip30: max |S_N - Phi S0 Phi^T| / max |S_N| = {worst:.2e} (measured {cvc.LIP_IDENTITY_MEASURED:.1e}, tolerance {cvc.LIP_IDENTITY_TOL:.1e})")
    assert worst <= cvc.LIP_IDENTITY_TOL


def test_the_recursion_reproduces_the_sigma_points_of_the_linearised_closed_loop():
    """2 nx sigma points +- sqrt(nx) L e_i of S0 = L L^T through A_k: their empirical covariance (mean zero, weights 1 / (2 nx)) is the
    recursion's S_steps.  Both are products of the same matrices in another order: the tolerance is 1e-12 of the entrywise magnitude
    |A| .. |S0| .. |A|^T, four orders above the rounding of 2 x 4 products of 13 x 13 (2 * 4 * 13 * 2^-53 = 1.2e-14)."""
    m, xs, us, P, K = _plan()
    nx = m.nx
    S0 = cvc.general_s0(nx, 4)
    L = np.linalg.cholesky(S0)
    pts = np.concatenate([np.sqrt(nx) * L, -np.sqrt(nx) * L], axis=1)      # columns
    mag = np.abs(S0)
    for k in range(M):
        A, _ = cvc.linearisation(m, xs, us, P, K, 1, k)
        pts = A @ pts
        mag = np.abs(A) @ mag @ np.abs(A).T
    emp = pts @ pts.T / (2 * nx)
    got = cvc.covariance_reference(m, xs, us, P, K, 1, S0, None, None, 0, M, ML)["cov"][M]
    err = np.abs(got - emp)
    print(f"srbd13: worst |recursion - sigma points| / magnitude = {float(np.max(err / mag)):.2e}")
    assert np.all(err <= 1e-12 * mag)


def test_the_cone_margin_in_sigmas_halves_when_the_covariance_quadruples():
    m, xs, us, P, K = _plan()
    S0 = cvc.general_s0(m.nx, 5)
    a = cvc.covariance_reference(m, xs, us, P, K, 1, S0, None, None, 0, M, ML)
    b = cvc.covariance_reference(m, xs, us, P, K, 1, 4.0 * S0, None, None, 0, M, ML)
    assert np.isfinite(a["record"][0]) and a["cone"] and b["record"][0] == 0.5 * a["record"][0]
    np.testing.assert_array_equal(b["cov"], 4.0 * a["cov"])
    np.testing.assert_array_equal(b["record"][1:4], a["record"][1:4])
    # the margin is the audit's cone word in another scale: for the rows with a side force, -a.f = -(+-f_xy - ml f_z) >= -(max|f_xy| - ml f_z)
    z, node, n, row, spread = min(a["cone"])
    assert (z, node, n, row) == (a["record"][0], *a["record"][1:4])
