"""Plan uncertainty on the device (include/sddp.h sddp_policy_covariance_device): the covariances against the rule of
tests/policy_covariance_cases.py, knot by knot from the device's own S_j, and the record recomputed from the device's own outputs, on
every kernel family; the linear model against the device's own policy rollout; exact scaling and range independence, bit for bit;
ok = 0; per-instance constants; nothing else moves; refusals; the fleet queue."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import models as omodels
from srbd_horizon_amd import _lib, workload
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.fleet import FleetQueue
from tests import plan_audit_cases as pac, policy_covariance_cases as cvc
from tests.gpu_support import assert_nothing_else_moves, dev as _dev, solve, solved
from tests.variant_cases import TRACKING, draw

pytestmark = pytest.mark.gpu

OPTS = pac.OPTS
W = _lib.POLICY_COV_WORDS


def _cov_dev(eng, S0, q=None, r=None, first=0, count=None, start=0, steps=None, friction=0.0, optional=True):
    """policy_covariance_device on fresh device tensors pre-filled with 7.0 -> numpy (record, cov, ucov_diag)"""
    n = eng.B - first if count is None else count
    s = eng.policy_words()[1] - start if steps is None else steps
    rows = max(s, 0)
    mk = lambda *shape: torch.full((n, *shape), 7.0, dtype=torch.float64, device="cuda")      # noqa: E731
    out, cov, ud = mk(W), mk(rows + 1, eng.nx, eng.nx) if optional else None, mk(rows, eng.nu) if optional else None
    eng.policy_covariance_device(_dev(S0), out, _dev(q), _dev(r), cov, ud, first, n, start, s, friction)
    eng.synchronize()
    return out.cpu().numpy(), None if cov is None else cov.cpu().numpy(), None if ud is None else ud.cpu().numpy()


def _inputs(eng, B, seed=0):
    """a full, non-diagonal S0 per instance, and q, r"""
    rng = np.random.default_rng(seed)
    S0 = np.array([cvc.general_s0(eng.nx, seed + 10 + b) for b in range(B)])
    return S0, 1e-6 * (0.5 + rng.random((B, eng.nx))), 1e-4 * (0.5 + rng.random((B, eng.nu)))


def _ml(eng, friction=0.0):
    return (friction if friction > 0.0 else eng.consts.friction_cone_coefficient) / np.sqrt(2.0)


def _check(model_of, eng, x, u, P, K, ok, S0, q, r, start, steps, got, label, friction=0.0):
    rec, cov, ud = got
    B = S0.shape[0]
    assert rec.shape == (B, W) and cov.shape == (B, steps + 1, eng.nx, eng.nx) and ud.shape == (B, steps, eng.nu)
    worst = 0.0
    for b in range(B):
        m = model_of(b)
        S = np.tril(S0[b]) + np.tril(S0[b], -1).T
        np.testing.assert_array_equal(cov[b, 0], S)
        worst = max(worst, cvc.assert_one_step(m, x[b], u[b], P[b], K[b], ok[b], None if q is None else q[b], None if r is None else r[b],
                                               start, cov[b], label=f"{label} instance {b}"))
        # diag U_j from the device's own S_j and the fetched K, at the tolerance of the record's words
        for j in range(steps):
            ref = np.einsum("rj,jl,rl->r", K[b][start + j], cov[b, j], K[b][start + j]) if ok[b] else np.zeros(eng.nu)
            mag = np.einsum("rj,jl,rl->r", np.abs(K[b][start + j]), np.abs(cov[b, j]), np.abs(K[b][start + j])) if ok[b] else np.zeros(eng.nu)
            assert np.all(np.abs(ud[b, j] - ref) <= cvc.RECORD_RTOL * mag), f"{label} instance {b} knot {start + j}: diag U"
        cvc.assert_record(m, u[b], P[b], K[b], ok[b], start, _ml(eng, friction), rec[b], cov[b], ud[b], label=f"{label} instance {b}")
    return worst


# srbd37: N = 6 is the shortest horizon the other inspectors' cases of tests/plan_audit_cases.py use for it
@pytest.mark.parametrize("model,N,B,wps", [("srbd13", 6, 5, 1), ("srbd13", 6, 5, 2), ("srbd37", 6, 3, None), ("lip30", 6, 3, None),
                                           ("srbd61", 4, 2, None)])
def test_covariances_and_record_match_the_rule(model, N, B, wps):
    eng, cst, batch, x, u, st, P = solved(model, N, B, wps=wps, knots=N)
    _, K, info = eng.policy()
    assert (info[:, 3] == 1.0).all()
    m = omodels.make_model(model, cst)
    S0, q, r = _inputs(eng, B)
    for start, steps in ((1, N - 1), (0, 1)):
        for qq, rr in ((q, r), (None, None)):
            got = _cov_dev(eng, S0, qq, rr, start=start, steps=steps)
            worst = _check(lambda b: m, eng, x, u, P, K, info[:, 3], S0, qq, rr, start, steps, got, f"{model} start {start} steps {steps}")
            print(f"{model} wps {wps} start {start} steps {steps} noise {qq is not None}: one-step error / bound {worst:.2e}; "
                  f"min z {got[0][:, 0]}")
            if model != "lip30":
                assert np.all(np.isfinite(got[0][:, 0]))                    # a stance force and a spread: the cone words are in play
    # the host-array form, steps None (to the last kept knot), and a friction coefficient of the call
    res = eng.policy_covariance(S0, q, r, start=1)
    ref = _cov_dev(eng, S0, q, r, start=1, steps=N - 1)
    assert res["record"].tobytes() == ref[0].tobytes() and res["cov"].tobytes() == ref[1].tobytes() and res["ucov_diag"].tobytes() == ref[2].tobytes()
    got = _cov_dev(eng, S0, q, r, start=1, friction=0.3)
    assert got[1].tobytes() == ref[1].tobytes()
    _check(lambda b: m, eng, x, u, P, K, info[:, 3], S0, q, r, 1, N - 1, got, f"{model} friction 0.3", friction=0.3)
    # without the optional outputs the record is the same bytes
    assert _cov_dev(eng, S0, q, r, start=1, optional=False)[0].tobytes() == ref[0].tobytes()
    n = C.c_int()
    assert eng.lib.sddp_policy_covariance_words(eng.h, C.byref(n)) == 0 and n.value == W


def test_on_the_linear_model_the_covariance_is_the_policy_rollouts_transition_matrix():
    """lip30 is linear, so the closed loop is affine and S_steps = Phi S0 Phi^T with Phi from sddp_policy_rollout_device columns at
    x_0 +- e_i: no oracle in the loop; the tolerance is the reference's own rounding of the identity x 10
    (tests/policy_covariance_cases.py LIP_IDENTITY_TOL)."""
    model, N, B = "lip30", 6, 3
    eng, cst, batch, x, u, st, P = solved(model, N, B, knots=N)
    S0, _, _ = _inputs(eng, B, seed=100)
    rec, cov, _ = _cov_dev(eng, S0)
    nx = eng.nx
    ends = []
    for sign in (1.0, -1.0):
        for i in range(nx):
            xm = x[:, 0].copy()
            xm[:, i] += sign
            ends.append(eng.policy_rollout(xm)[0][:, N])
    ends = np.array(ends)                                                   # [2 nx, B, nx]
    worst = 0.0
    for b in range(B):
        Phi = ((ends[:nx, b] - ends[nx:, b]) / 2.0).T
        worst = max(worst, cvc.identity_error(cov[b, N], Phi, S0[b]))
    print(f"lip30: max |S_N - Phi S0 Phi^T| / max |S_N| = {worst:.2e} (tolerance {cvc.LIP_IDENTITY_TOL:.1e})")
    assert worst <= cvc.LIP_IDENTITY_TOL
    assert np.all(rec[:, 0] == np.inf) and np.all(rec[:, 1:4] == -1)


def test_exact_properties_bit_for_bit():
    model, N, B = "srbd13", 6, 5
    eng, cst, batch, x, u, st, P = solved(model, N, B, knots=N)
    S0, q, r = _inputs(eng, B)
    zero = _cov_dev(eng, np.zeros_like(S0))
    assert not zero[1].any() and not zero[2].any() and np.all(zero[0][:, 0] == np.inf) and np.all(zero[0][:, 1:4] == -1)
    one, four = _cov_dev(eng, S0), _cov_dev(eng, 4.0 * S0)
    assert four[1].tobytes() == (4.0 * one[1]).tobytes() and four[2].tobytes() == (4.0 * one[2]).tobytes()
    assert np.all(np.isfinite(one[0][:, 0])) and four[0][:, 0].tobytes() == (0.5 * one[0][:, 0]).tobytes()
    np.testing.assert_array_equal(four[0][:, 1:4], one[0][:, 1:4])
    # the result of an instance does not depend on the range it was part of, nor on what ran in between
    whole = _cov_dev(eng, S0, q, r)
    part = _cov_dev(eng, S0[1:4], q[1:4], r[1:4], first=1, count=3)
    eng.audit()                                                            # an unrelated launch
    again = _cov_dev(eng, S0, q, r)
    for i in range(3):
        assert part[i].tobytes() == whole[i][1:4].tobytes() and again[i].tobytes() == whole[i].tobytes()


def test_without_a_policy_launch_the_propagation_is_open_loop():
    model, N, B = "srbd13", 6, 5
    batch, P, consts, opts = pac.problem(model, N, B, "plain")
    eng = DdpEngine(model, N, B, opts=opts, consts=consts)
    eng.enable_policy(N)
    x, u, _ = solve(eng, batch, P)
    assert not eng.fetch_policy().any()                                    # zero records: ok = 0
    m = omodels.make_model(model, omodels.RobotConsts(**consts))
    S0, q, r = _inputs(eng, B)
    K = np.full((B, N, eng.nu, eng.nx), np.nan)                            # never read
    for start, steps in ((0, N), (1, N - 1)):
        got = _cov_dev(eng, S0, q, r, start=start, steps=steps)
        _check(lambda b: m, eng, x, u, P, K, np.zeros(B), S0, q, r, start, steps, got, f"ok = 0 start {start}")
        assert not got[2].any() and np.all(got[0][:, 0] == np.inf) and np.all(got[0][:, 1:4] == -1) and np.all(got[0][:, 14] == 0.0)
        assert np.all(got[0][:, 9] == 0.0)
    eng.close()


def test_each_robot_is_linearised_through_its_own_constants():
    model, N, B = "srbd13", 6, 2
    batch = workload.make_batch(model, N, np.arange(B) + 3)
    over, csts = draw(batch["consts"], B, TRACKING, seed=3)
    over["m"], over["dt"] = np.array([30.0, 55.0]), np.array([0.03, 0.06])
    csts = [dataclasses.replace(c, m=float(mm), dt=float(d)) for c, mm, d in zip(csts, over["m"], over["dt"])]
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    eng.set_instance_consts(over)
    eng.enable_policy(N)
    x, u, _ = solve(eng, batch)
    eng.policy_range_device()
    _, K, info = eng.policy()
    assert (info[:, 3] == 1.0).all()
    S0, q, r = _inputs(eng, B)
    got = _cov_dev(eng, S0, q, r)
    models = [omodels.make_model(model, c) for c in csts]
    _check(lambda b: models[b], eng, x, u, batch["params"], K, info[:, 3], S0, q, r, 0, N, got, "own robots")
    common = omodels.make_model(model, omodels.RobotConsts(**batch["consts"]))
    apart = max(float(np.max(np.abs(got[1][b] - cvc.covariance_reference(common, x[b], u[b], batch["params"][b], K[b], 1, S0[b], q[b], r[b], 0, N,
                                                                       _ml(eng))["cov"]) / np.max(np.abs(got[1][b])))) for b in range(B))
    print(f"own robots against the handle's robot: relative distance of the covariances {apart:.3e}")
    assert apart > 1e-6
    eng.close()


def test_nothing_else_moves():
    def touch(eng, batch, x):
        S0, q, r = _inputs(eng, eng.B)
        got = (*_cov_dev(eng, S0, q, r), *_cov_dev(eng, S0[1:4], None, None, first=1, count=3, start=1), eng.policy_covariance(S0)["record"])
        return tuple(a.tobytes() for a in got)

    assert_nothing_else_moves(touch, OPTS, policy=True)


def test_refusals():
    model, N, B, M = "srbd13", 6, 2, 3
    batch = workload.make_batch(model, N, [0, 1])
    eng = DdpEngine(model, N, B, opts=OPTS)
    S0 = np.array([cvc.general_s0(eng.nx, b) for b in range(B)])
    kept = []

    def call(first=0, count=B, start=0, steps=M):
        """the call on outputs pre-filled with 7.0, which a refusal must leave alone"""
        mk = lambda *shape: torch.full((max(count, 0), *shape), 7.0, dtype=torch.float64, device="cuda")      # noqa: E731
        out, cov, ud = mk(W), mk(max(steps, 0) + 1, eng.nx, eng.nx), mk(max(steps, 0), eng.nu)
        kept[:] = [out, cov, ud]
        eng.policy_covariance_device(_dev(S0[:max(count, 0)]), out, None, None, cov, ud, first, count, start, steps)
        eng.synchronize()
        return out.cpu().numpy()

    def refused(match, **kw):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
        eng.synchronize()
        assert all(bool((t == 7.0).all()) for t in kept), (match, kw)

    refused("sddp_enable_policy")                                          # no policy buffer
    eng.enable_policy(M)
    refused("no solve has run")
    solve(eng, batch)
    eng.policy_range_device()
    for start, steps in ((0, M + 1), (1, M), (M, 1), (-1, 1), (0, 0)):
        refused(f"start \\+ steps <= {M}", start=start, steps=steps)
    refused("range outside", first=1, count=2)
    d_s0 = _dev(S0)
    out = torch.full((B, W), 7.0, dtype=torch.float64, device="cuda")
    for s0p, outp in ((None, eng._dev(out, out.shape)), (eng._dev(d_s0, d_s0.shape), None)):
        rc = eng.lib.sddp_policy_covariance_device(eng.h, 0, B, 0, M, s0p, None, None, 0.0, outp, None, None)
        assert rc == -1                                                    # SDDP_ERR_ARG
        with pytest.raises(RuntimeError, match="NULL argument"):
            eng._chk(rc)
    eng.synchronize()
    assert bool((out == 7.0).all())
    assert call().shape == (B, W) and not (kept[1] == 7.0).any()           # and the handle still works
    eng.close()
    # every build without a policy kernel: sddp_enable_policy refuses, so the call finds no policy buffer
    for e in (DdpEngine(model, N, B, opts=dict(OPTS, second_order=2)),
              DdpEngine("srbd37", 6, 1, opts=OPTS, consts=dict(friction_barrier_weight=1e-3, friction_barrier_sharpness=5.0))):
        with pytest.raises(RuntimeError, match="no policy kernel"):
            e.enable_policy(1)
        out = torch.full((e.B, W), 7.0, dtype=torch.float64, device="cuda")
        s0 = torch.zeros((e.B, e.nx, e.nx), dtype=torch.float64, device="cuda")
        rc = e.lib.sddp_policy_covariance_device(e.h, 0, e.B, 0, 1, e._dev(s0, s0.shape), None, None, 0.0, e._dev(out, out.shape), None, None)
        assert rc == -1 and b"sddp_enable_policy" in e.lib.sddp_last_error(e.h)
        e.synchronize()
        assert bool((out == 7.0).all())
        e.close()


def test_fleet_queue_follows_the_last_flush():
    model, N, batch_n, depth = "srbd13", 6, 4, 2
    batch = workload.make_batch(model, N, np.arange(batch_n) + 3)
    eng = DdpEngine(model, N, batch_n * depth, opts=OPTS, consts=batch["consts"])
    eng.enable_policy(N)
    t = {k: _dev(batch[k]) for k in ("x0", "xs", "us", "params")}
    fleet = FleetQueue(eng, t["params"].repeat(depth, 1, 1).contiguous(), batch_n, depth, gather="first_knot", policy=True)
    total = batch_n * depth
    S0 = _dev(np.array([cvc.general_s0(eng.nx, b % batch_n) for b in range(total + 1)]))
    out = torch.full((total + 1, W), 7.0, dtype=torch.float64, device="cuda")
    cov = torch.full((total + 1, N, eng.nx, eng.nx), 7.0, dtype=torch.float64, device="cuda")      # start = 1: N - 1 steps
    assert fleet.policy_covariance(S0, out) == 0                           # nothing flushed yet: nothing launched
    assert bool((out == 7.0).all())
    fleet.submit(t["x0"], t["xs"], t["us"])
    assert fleet.flush() == batch_n and fleet.policy_covariance(S0, out) == batch_n      # a partial handle: the first block alone
    eng.synchronize()
    got = out.cpu().numpy()
    ref = _cov_dev(eng, S0[:batch_n].cpu().numpy(), first=0, count=batch_n)
    assert got[:batch_n].tobytes() == ref[0].tobytes() and np.all(got[batch_n:] == 7.0) and np.all(got[:batch_n, 14] == 1.0)
    fleet.submit(t["x0"], t["xs"], t["us"])
    fleet.submit(t["x0"], t["xs"], t["us"])
    assert fleet.flush() == total and fleet.policy_covariance(S0, out, cov=cov, start=1) == total
    eng.synchronize()
    got, gcov = out.cpu().numpy(), cov.cpu().numpy()
    ref = _cov_dev(eng, S0[:total].cpu().numpy(), start=1)
    assert got[:-1].tobytes() == ref[0].tobytes() and np.all(got[-1] == 7.0)
    assert gcov[:total].tobytes() == ref[1].tobytes() and np.all(gcov[total] == 7.0)
    assert got[:batch_n].tobytes() == got[batch_n:2 * batch_n].tobytes()   # the same robots in both blocks
    eng.close()
