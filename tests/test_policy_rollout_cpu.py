"""Policy rollout (include/sddp.h sddp_apply_policy_knot_device, sddp_policy_rollout_device), what needs no GPU: the parameter names
of the two declarations, the engine's methods, and the rule of tests/policy_rollout_cases.py on the oracle alone."""
import functools
import inspect

import numpy as np

from oracle import ddp as oddp, models as omodels
from srbd_horizon_amd import workload
from srbd_horizon_amd.engine import DdpEngine
from tests import abi_header, policy_cases as pc, policy_rollout_cases as prc
from tests.oracle_refs import frozen

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
M = 4


def test_header_and_ctypes_agree_on_the_two_symbols():
    """the order of the integers, which no type tells apart, and what is read-only (the types: tests/test_abi.py, for every symbol)"""
    declared = abi_header.functions()
    assert declared["sddp_apply_policy_knot_device"][1][:5] == ["sddp_handle* h", "int first", "int count", "int knot", "const double* d_x_meas"]
    assert declared["sddp_policy_rollout_device"][1][:6] == ["sddp_handle* h", "int first", "int count", "int start", "int steps", "const double* d_x_meas"]


def test_engine_methods_and_defaults():
    sig = inspect.signature(DdpEngine.apply_policy_device)
    assert list(sig.parameters) == ["self", "x_meas", "u_out", "first", "count", "knot"] and sig.parameters["knot"].default == 0
    sig = inspect.signature(DdpEngine.policy_rollout_device)
    assert list(sig.parameters) == ["self", "x_meas", "x_out", "u_out", "cost_out", "first", "count", "start", "steps"]
    assert sig.parameters["cost_out"].default is None and sig.parameters["start"].default == 0 and sig.parameters["steps"].default is None
    sig = inspect.signature(DdpEngine.policy_rollout)
    assert list(sig.parameters) == ["self", "x_meas", "first", "count", "start", "steps"]
    assert sig.parameters["start"].default == 0 and sig.parameters["steps"].default is None


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


def _open_loop(m, us, P, x_meas, start, steps):
    x, cost = [x_meas], 0.0
    for k in range(start, start + steps):
        cost += m.cost(x[-1], us[k], P[k], k)
        x.append(m.f(x[-1], us[k], P[k]))
    return np.array(x), cost


def test_ok_zero_is_the_open_loop_rollout():
    m, xs, us, P, K = _plan()
    xm = xs[1] + 1e-3 * np.random.default_rng(0).standard_normal(m.nx)
    x, u, cost = prc.rollout_reference(m, xs, us, P, np.full_like(K, np.nan), 0, xm, 1, M - 1)      # (ok = 0: K is never read)
    xo, co = _open_loop(m, us, P, xm, 1, M - 1)
    np.testing.assert_array_equal(x, xo)
    np.testing.assert_array_equal(u, us[1:M])
    assert cost == co


def test_from_the_plans_own_state_the_first_input_is_the_plans():
    m, xs, us, P, K = _plan()
    for start in (0, 2):
        x, u, _ = prc.rollout_reference(m, xs, us, P, K, 1, xs[start], start, M - start)
        np.testing.assert_array_equal(u[0], us[start])
        np.testing.assert_array_equal(x[0], xs[start])


def test_the_reference_shadows_itself():
    m, xs, us, P, K = _plan()
    xm = xs[0] + 1e-2 * np.random.default_rng(1).standard_normal(m.nx)
    for ok in (1, 0):
        x, u, cost = prc.rollout_reference(m, xs, us, P, K, ok, xm, 0, M)
        assert prc.assert_rollout_shadows(m, xs, us, P, K, ok, 0, x, u, cost) == (0.0, 0.0, 0.0)


def test_feedback_brings_a_pushed_state_nearer_the_plan():
    """direction only: a push of 1e-3 on the lateral CoM velocity, the state at the last knot with and without K"""
    m, xs, us, P, K = _plan()
    xm = xs[0].copy()
    xm[8] += 1e-3
    xc, _, _ = prc.rollout_reference(m, xs, us, P, K, 1, xm, 0, M)
    xo, _, _ = prc.rollout_reference(m, xs, us, P, K, 0, xm, 0, M)
    dc, do = np.linalg.norm(xc[M] - xs[M]), np.linalg.norm(xo[M] - xs[M])
    print(f"distance from the plan at knot {M}: closed loop {dc:.3e}, open loop {do:.3e}")
    assert dc < do
