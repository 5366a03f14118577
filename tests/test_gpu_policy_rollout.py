"""The later knots of the exported policy on the device (include/sddp.h sddp_apply_policy_knot_device, sddp_policy_rollout_device):
the rollout against the rule of tests/policy_rollout_cases.py, knot by knot from the device's own states, on every kernel family
and the "_x" build; bit identities among the device entry points; per-instance constants; ok = 0; nothing else moves; refusals."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import models as omodels
from srbd_horizon_amd import workload
from srbd_horizon_amd.engine import DdpEngine
from tests import policy_rollout_cases as prc
from tests.gpu_support import assert_nothing_else_moves, dev as _dev, frozen, solve
from tests.variant_cases import TRACKING, draw, extra_rows_problem

pytestmark = pytest.mark.gpu

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)      # tests/test_gpu_policy.py


def _rollout_dev(eng, xm, first=0, count=None, start=0, steps=None, cost=True):
    """policy_rollout_device on fresh device tensors -> numpy (x, u, cost or None)"""
    n = eng.B - first if count is None else count
    s = eng.policy_words()[1] - start if steps is None else steps
    x = torch.full((n, s + 1, eng.nx), np.nan, dtype=torch.float64, device="cuda")
    u = torch.full((n, s, eng.nu), np.nan, dtype=torch.float64, device="cuda")
    c = torch.full((n,), np.nan, dtype=torch.float64, device="cuda") if cost else None
    eng.policy_rollout_device(_dev(xm), x, u, c, first, n, start, s)
    eng.synchronize()
    return x.cpu().numpy(), u.cpu().numpy(), None if c is None else c.cpu().numpy()


def _apply(eng, xm, first=0, count=None, **kw):
    n = eng.B - first if count is None else count
    out = torch.full((n, eng.nu), np.nan, dtype=torch.float64, device="cuda")
    eng.apply_policy_device(_dev(xm), out, first, n, **kw)
    eng.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _solved(model, N, B, M, xr=False, policy=True):
    """a handle with its solve and (policy=True) its policy launch done, and what they gave: computed once, arrays read-only"""
    seeds = np.arange(B) + 3
    if xr:
        batch, P, consts = extra_rows_problem(model, N, seeds)
    else:
        batch = workload.make_batch(model, N, seeds)
        P, consts = batch["params"], batch["consts"]
    eng = DdpEngine(model, N, B, opts=OPTS, consts=consts)
    eng.enable_policy(M)
    x, u, st = solve(eng, batch, P)
    if policy:
        eng.policy_range_device()
    _, K, info = eng.policy()
    return (eng, consts, *frozen((x, u, P, K, info)))


def _pushed(x, start, seed=7, size=1e-2):
    return x[:, start] + size * np.random.default_rng(seed).standard_normal(x[:, start].shape)


@pytest.mark.parametrize("model,N,B,M,xr", [("srbd13", 6, 5, 4, False), ("srbd37", 6, 3, 3, False), ("lip30", 6, 3, 3, False),
                                            ("srbd61", 4, 2, 2, False), ("srbd13", 6, 3, 3, True)])
def test_rollout_shadows_the_oracle(model, N, B, M, xr):
    eng, consts, x, u, P, K, info = _solved(model, N, B, M, xr)
    assert (info[:, 3] == 1.0).all()
    m = omodels.make_model(model, omodels.RobotConsts(**consts))
    for start, steps in ((0, M), (0, 1), (1, M - 1)):
        xm = _pushed(x, start)
        gx, gu, gc = eng.policy_rollout(xm, start=start, steps=steps)
        assert gx.shape == (B, steps + 1, eng.nx) and gu.shape == (B, steps, eng.nu) and gc.shape == (B,)
        np.testing.assert_array_equal(gx[:, 0], xm)
        worst = np.max([prc.assert_rollout_shadows(m, x[b], u[b], P[b], K[b], 1, start, gx[b], gu[b], gc[b],
                                                   label=f"{model} instance {b} start {start} steps {steps}") for b in range(B)], axis=0)
        print(f"{model}{' _x' if xr else ''} start {start} steps {steps}: input error / bound {worst[0]:.2e}, state rel {worst[1]:.2e}, "
              f"cost rel {worst[2]:.2e}")
    gx2, gu2, gc2 = eng.policy_rollout(_pushed(x, 1), start=1)           # steps None: to the last kept knot
    np.testing.assert_array_equal(gx2, gx); np.testing.assert_array_equal(gu2, gu); np.testing.assert_array_equal(gc2, gc)


@pytest.mark.parametrize("model,N,B,M", [("srbd13", 6, 70, 4), ("srbd37", 6, 3, 3)])
def test_bit_identities_among_the_device_entry_points(model, N, B, M):
    eng, consts, x, u, P, K, info = _solved(model, N, B, M)
    xm0 = _pushed(x, 0)
    old = _apply(eng, xm0)                                                                 # the call as it was: sddp_apply_policy_device
    assert _apply(eng, xm0, knot=0).tobytes() == old.tobytes()
    d_xm0, knot0 = _dev(xm0), torch.full((B, eng.nu), np.nan, dtype=torch.float64, device="cuda")
    eng._chk(eng.lib.sddp_apply_policy_knot_device(eng.h, 0, B, 0, eng._dev(d_xm0, (B, eng.nx)), eng._dev(knot0, (B, eng.nu))))      # the new symbol
    eng.synchronize()
    assert knot0.cpu().numpy().tobytes() == old.tobytes()
    ref = u[:, 0] + np.einsum("bij,bj->bi", K[:, 0], xm0 - x[:, 0])                        # and it is the policy, not u_0 alone
    assert np.max(np.abs(old - ref)) <= 1e-12 * np.max(np.abs(K[:, 0])) * np.max(np.abs(xm0 - x[:, 0])) * eng.nx < np.max(np.abs(old - u[:, 0]))
    for s in range(M):
        xm = _pushed(x, s)
        gx, gu, gc = _rollout_dev(eng, xm, start=s)
        assert gu[:, 0].tobytes() == _apply(eng, xm, knot=s).tobytes(), f"start {s}"
        # Both kernels inline the same M::step on the same operands, but not provably as the same instruction sequence: model_step_kernel
        # discards the stage cost that policy_rollout_kernel accumulates, and the cost shares products with the dynamics (wdot), so
        # under the compiler's free contraction a product may be fused into an FMA in one kernel and kept apart in the other.  Bit
        # equality is therefore reported; asserted is agreement within one rounding of each component: one unit in its last place.
        step = eng.model_step(xm, gu[:, 0], P[:, s], s)
        ulps = float(np.max(np.abs(gx[:, 1] - step) / np.spacing(np.abs(step))))
        print(f"{model} start {s}: x_out[:, 1] bit-equal to model_step: {gx[:, 1].tobytes() == step.tobytes()}; worst difference {ulps:.0f} ulp")
        assert ulps <= 1.0, (model, s, ulps)
    # ranges: the result of an instance does not depend on the range it was part of
    xm = _pushed(x, 0)
    whole = _rollout_dev(eng, xm)
    cut = 20 if B > 20 else 1
    a, b_ = _rollout_dev(eng, xm[:cut], 0, cut), _rollout_dev(eng, xm[cut:], cut, B - cut)
    for i in range(3):
        assert np.concatenate([a[i], b_[i]]).tobytes() == whole[i].tobytes()
    f, c = (5, 3) if B > 8 else (1, 2)
    part = _rollout_dev(eng, xm[f:f + c], f, c)
    for i in range(3):
        assert part[i].tobytes() == whole[i][f:f + c].tobytes()
    nocost = _rollout_dev(eng, xm, cost=False)                                             # d_cost_out = NULL
    assert nocost[2] is None and nocost[0].tobytes() == whole[0].tobytes() and nocost[1].tobytes() == whole[1].tobytes()
    # the table form: a table of B copies of the handle's own constants
    batch = workload.make_batch(model, N, np.arange(B) + 3)
    tab = DdpEngine(model, N, B, opts=OPTS, consts=consts)
    tab.set_instance_consts({"m": np.full(B, tab.consts.m)})
    tab.enable_policy(M)
    x2, u2, _ = solve(tab, batch)
    tab.policy_range_device()
    assert tab.instance_consts_active()
    assert x2.tobytes() == x.tobytes() and u2.tobytes() == u.tobytes() and tab.fetch_policy().tobytes() == eng.fetch_policy().tobytes()
    got = _rollout_dev(tab, xm)
    for i in range(3):
        assert got[i].tobytes() == whole[i].tobytes()
    assert _apply(tab, xm, knot=M - 1).tobytes() == _apply(eng, xm, knot=M - 1).tobytes()
    tab.close()


def test_rollout_uses_each_robots_own_constants():
    model, N, B, M = "srbd13", 6, 6, 4
    batch = workload.make_batch(model, N, np.arange(B) + 3)
    over, csts = draw(batch["consts"], B, TRACKING, seed=3)
    over["dt"] = np.linspace(0.02, 0.06, B)
    csts = [dataclasses.replace(c, dt=float(d)) for c, d in zip(csts, over["dt"])]
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    eng.set_instance_consts(over)
    eng.enable_policy(M)
    x, u, _ = solve(eng, batch)
    eng.policy_range_device()
    _, K, info = eng.policy()
    assert (info[:, 3] == 1.0).all()
    xm = _pushed(x, 0)
    gx, gu, gc = eng.policy_rollout(xm)
    common = omodels.make_model(model, omodels.RobotConsts(**batch["consts"]))
    apart = 0.0
    for b in range(B):
        prc.assert_rollout_shadows(omodels.make_model(model, csts[b]), x[b], u[b], batch["params"][b], K[b], 1, 0, gx[b], gu[b], gc[b],
                                   label=f"robot {b}")
        apart = max(apart, float(np.max(np.abs(gx[b] - prc.rollout_reference(common, x[b], u[b], batch["params"][b], K[b], 1, xm[b], 0, M)[0]))))
    print(f"own robots against the handle's robot: max |x' - x'_common| = {apart:.3e}")
    assert apart > 1e-6


def test_without_a_policy_launch_the_rollout_is_open_loop():
    model, N, B, M = "srbd13", 6, 5, 4
    eng, consts, x, u, P, K, info = _solved(model, N, B, M, False, False)
    assert not eng.fetch_policy().any()                                                    # zero records: ok = 0
    m = omodels.make_model(model, omodels.RobotConsts(**consts))
    for start, steps in ((0, M), (1, M - 1)):
        xm = _pushed(x, start)
        gx, gu, gc = eng.policy_rollout(xm, start=start, steps=steps)
        np.testing.assert_array_equal(gx[:, 0], xm)
        np.testing.assert_array_equal(gu, u[:, start:start + steps])
        for b in range(B):
            prc.assert_rollout_shadows(m, x[b], u[b], P[b], None, 0, start, gx[b], gu[b], gc[b], label=f"instance {b}")
    np.testing.assert_array_equal(_apply(eng, _pushed(x, 1), knot=1), u[:, 1])


def test_nothing_else_moves():
    def touch(eng, batch, x):
        xm, M = _pushed(x, 0), eng.knots
        got = (*_rollout_dev(eng, xm), _apply(eng, xm, knot=M - 1), _apply(eng, xm, knot=1))
        return tuple(a.tobytes() for a in got)

    assert_nothing_else_moves(touch, OPTS, policy=True)


def test_rollout_refusals():
    model, N, B, M = "srbd13", 6, 2, 3
    batch = workload.make_batch(model, N, [0, 1])
    eng = DdpEngine(model, N, B, opts=OPTS)
    xm = batch["x0"]

    def rollout(first=0, count=B, start=0, steps=M):
        return _rollout_dev(eng, xm[:count], first, count, start, steps)

    with pytest.raises(RuntimeError, match="sddp_enable_policy"):                     # no policy buffer
        rollout()
    with pytest.raises(RuntimeError, match="sddp_enable_policy"):
        _apply(eng, xm, knot=1)
    eng.enable_policy(M)
    with pytest.raises(RuntimeError, match="no solve has run"):                       # a rollout before any solve
        rollout()
    solve(eng, batch)
    eng.policy_range_device()
    for knot in (M, -1):
        with pytest.raises(RuntimeError, match=f"0 <= knot < {M}"):
            _apply(eng, xm, knot=knot)
    for start, steps in ((0, M + 1), (1, M), (M, 1), (-1, 1), (0, 0)):
        with pytest.raises(RuntimeError, match=f"start \\+ steps <= {M}"):
            rollout(start=start, steps=steps)
    with pytest.raises(RuntimeError, match="range outside"):
        rollout(first=1, count=2)
    with pytest.raises(RuntimeError, match="range outside"):
        _apply(eng, xm, first=1, count=2, knot=1)
    with pytest.raises(RuntimeError, match="NULL argument"):
        eng._chk(eng.lib.sddp_policy_rollout_device(eng.h, 0, B, 0, M, None, None, None, None))
    assert rollout()[0].shape == (B, M + 1, eng.nx)                                   # and the handle still works
    so2 = DdpEngine(model, N, B, opts=dict(OPTS, second_order=2))                     # as in test_policy_refusals: nothing new is refused
    with pytest.raises(RuntimeError, match="no policy kernel"):
        so2.enable_policy(1)
    bar = DdpEngine("srbd37", 6, 1, opts=OPTS, consts=dict(friction_barrier_weight=1e-3, friction_barrier_sharpness=5.0))
    with pytest.raises(RuntimeError, match="no policy kernel"):
        bar.enable_policy(1)
