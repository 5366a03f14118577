"""Plan audit on the device (include/sddp.h sddp_audit_range_device, sddp_audit): the record of every kernel family, the "_x", the
barrier and the second_order = 2 build against the numpy statement of tests/plan_audit_cases.py on the device's own fetched x, u, P.

Tolerances (tests/plan_audit_cases.py assert_record):
  * words 0, 3, 5 - 9 are sums of at most three products of fetched numbers: 8 eps x the absolute operand sum the reference returns;
  * word 10 goes through the model step f: 10 x the largest disagreement between oracle.models' f and the C port's f
    (oracle/cport.py eval_knot) on the same (x_k, u_k, p_k).  Measured on the CPU over these cases (plan_audit_cases.CASES): at most
    9.03e-17 on the solved plans, at most 2.23e-16 on copies of them pushed by 1e-2 per state entry (what the audited policy rollouts
    visit).  F_DISAGREEMENT = 2.220446049250313e-16, so the tolerance is 2.22e-15, absolute;
  * an index word: the reference's candidate at the reported place is within the word's tolerance of the reference's maximum;
  * words 12 - 15 exactly.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import models as omodels
from srbd_horizon_amd import _lib, workload
from srbd_horizon_amd.engine import DdpEngine
from tests import plan_audit_cases as pac
from tests.gpu_support import (AUDIT, assert_common_refusals, assert_fleet_queue_follows_the_last_flush, assert_nothing_else_moves, dev,
                               solve, solved, touch_with)
from tests.variant_cases import TRACKING, draw

pytestmark = pytest.mark.gpu

A = _lib
W = _lib.AUDIT_WORDS


def _audit_dev(eng, first=0, count=None, **kw):
    """audit_device on a fresh device tensor -> numpy [count, 16]"""
    return AUDIT.device(eng, first, count, **kw)[0]


def _solved(model, N, B, kind, knots=0):
    eng, cst, batch, x, u, st, P = solved(model, N, B, kind, knots=knots)
    return eng, cst, x, u, P


def _check(model, cst, got, x, u, P, start, friction, label):
    m = omodels.make_model(model, cst)
    worst = np.zeros(2)
    for b in range(got.shape[0]):
        rec, ops, values = pac.audit_reference(m, x[b], u[b], P[b], start, friction)
        worst = np.maximum(worst, pac.assert_record(got[b], rec, ops, values, start, pac.DEFECT_TOL, label=f"{label} instance {b}"))
    print(f"{label}: worst error / tolerance, direct words {worst[0]:.3f}, defect {worst[1]:.3f}")


@pytest.mark.parametrize("model,N,B,kind", pac.CASES)
def test_the_solved_plan_against_the_reference(model, N, B, kind):
    eng, cst, x, u, P = _solved(model, N, B, kind)
    got = eng.audit()
    assert got.shape == (B, W) and got.dtype == np.float64
    print(f"{model} {kind}: cone {got[:, A.AUDIT_CONE]}, pull {got[:, A.AUDIT_PULL]}, defect {got[:, A.AUDIT_DEFECT]}")
    _check(model, cst, got, x, u, P, 0, cst.friction_cone_coefficient, f"{model} {kind}")
    assert _audit_dev(eng).tobytes() == got.tobytes()                           # the device entry point, on the caller's tensor
    if model == "lip30":
        assert np.all(np.isneginf(got[:, [A.AUDIT_CONE, A.AUDIT_PULL]])) and np.all(got[:, [1, 2, 4]] == -1.0)
        assert not got[:, [A.AUDIT_SWING_LOAD, A.AUDIT_QUAT_DRIFT, A.AUDIT_STANCE_PAIRS]].any()
    if model == "srbd13":
        assert not got[:, [A.AUDIT_FOOT_HEIGHT, A.AUDIT_SLIP, A.AUDIT_RIGID_FOOT]].any()


def test_an_instance_does_not_depend_on_its_range():
    eng, cst, x, u, P = _solved("srbd13", 6, 70, "plain")
    whole = eng.audit()
    _check("srbd13", cst, whole, x, u, P, 0, cst.friction_cone_coefficient, "srbd13 B = 70")
    for first, count in ((3, 64), (67, 3)):
        assert eng.audit(first, count).tobytes() == whole[first:first + count].tobytes()
        assert _audit_dev(eng, first, count).tobytes() == whole[first:first + count].tobytes()


def _pushed_rollout(eng, x, M, steps):
    """the policy rollout of pushed states from node 1, left on the device: (x' [B, steps + 1, nx], u' [B, steps, nu])"""
    xm = x[:, 1] + 1e-2 * np.random.default_rng(7).standard_normal(x[:, 1].shape)
    gx = torch.empty((eng.B, steps + 1, eng.nx), dtype=torch.float64, device="cuda")
    gu = torch.empty((eng.B, steps, eng.nu), dtype=torch.float64, device="cuda")
    eng.policy_rollout_device(dev(xm), gx, gu, None, 0, eng.B, 1, steps)
    return gx, gu


@pytest.mark.parametrize("model,N,B,M", [("srbd13", 6, 5, 4), ("srbd37", 6, 3, 3)])
def test_a_callers_trajectory(model, N, B, M):
    eng, cst, x, u, P = _solved(model, N, B, "plain", M)
    for steps in (M - 1, 1):
        gx, gu = _pushed_rollout(eng, x, M, steps)
        got = _audit_dev(eng, x=gx, u=gu, start=1, steps=steps)
        assert np.all(got[:, A.AUDIT_NODES] == steps)
        _check(model, cst, got, gx.cpu().numpy(), gu.cpu().numpy(), P, 1, cst.friction_cone_coefficient, f"{model} rollout, {steps} steps from node 1")
        part = _audit_dev(eng, 1, B - 1, x=gx[1:].contiguous(), u=gu[1:].contiguous(), start=1, steps=steps)      # block i is instance first + i
        assert part.tobytes() == got[1:].tobytes()
    # a NaN planted in the caller's u reaches exactly the words that read it
    gx, gu = _pushed_rollout(eng, x, M, M - 1)
    f_x = 0 if model == "srbd13" else 3                                          # f_x of contact 0
    gu[1, 1, f_x] = np.nan
    got = _audit_dev(eng, x=gx, u=gu, start=1, steps=M - 1)
    hx, hu = gx.cpu().numpy(), gu.cpu().numpy()
    _check(model, cst, got, hx, hu, P, 1, cst.friction_cone_coefficient, f"{model} rollout with a NaN")
    stance = P[1, 2, omodels.MODELS[model].P_SW[0] if model == "srbd13" else omodels.MODELS[model].p_sw(0)] > 0.5      # node 1 + 1
    reads = sorted([A.AUDIT_CONE if stance else A.AUDIT_SWING_LOAD, A.AUDIT_DEFECT])
    assert sorted(np.flatnonzero(np.isnan(got[1]))) == reads and not np.isnan(np.delete(got, 1, axis=0)).any()
    assert got[1, A.AUDIT_DEFECT_NODE] == -1 and (not stance or (got[1, A.AUDIT_CONE_NODE], got[1, A.AUDIT_CONE_CONTACT]) == (-1, -1))


def test_the_friction_argument():
    eng, cst, x, u, P = _solved("srbd13", 6, 5, "plain")
    own = eng.audit()
    for f in (0.0, -1.0, float("nan"), cst.friction_cone_coefficient):           # <= 0 or NaN: the handle's coefficient
        assert eng.audit(friction=f).tobytes() == own.tobytes(), f
        assert _audit_dev(eng, friction=f).tobytes() == own.tobytes(), f
    ice = eng.audit(friction=0.1)
    _check("srbd13", cst, ice, x, u, P, 0, 0.1, "srbd13 on ice")
    assert np.all(ice[:, A.AUDIT_CONE] != own[:, A.AUDIT_CONE])                  # word 0 follows the coefficient of the call
    assert ice[:, 3:].tobytes() == own[:, 3:].tobytes()                          # and no other word moves (1, 2: the place may)


def test_each_instance_is_stepped_through_its_own_robot():
    model, N, B = "srbd13", 6, 6
    batch = workload.make_batch(model, N, np.arange(B) + 3)
    over, csts = draw(batch["consts"], B, TRACKING, seed=3)
    over["dt"] = np.linspace(0.02, 0.06, B)
    csts = [dataclasses.replace(c, dt=float(d)) for c, d in zip(csts, over["dt"])]
    eng = DdpEngine(model, N, B, opts=pac.OPTS, consts=batch["consts"])
    eng.set_instance_consts(over)
    x, u, _ = solve(eng, batch)
    got = eng.audit()
    common = omodels.make_model(model, omodels.RobotConsts(**batch["consts"]))
    for b in range(B):
        _check(model, csts[b], got[b:b + 1], x[b:b + 1], u[b:b + 1], batch["params"][b:b + 1], 0, csts[b].friction_cone_coefficient, f"robot {b}")
        miss = abs(got[b, A.AUDIT_DEFECT] - pac.audit_reference(common, x[b], u[b], batch["params"][b], 0, 0.8)[0][A.AUDIT_DEFECT])
        print(f"robot {b}: defect {got[b, A.AUDIT_DEFECT]:.3e}; the handle's own robot misses it by {miss:.3e}")
        assert miss > pac.DEFECT_TOL
    eng.close()


def test_nothing_else_moves():
    sub_range_and_warm_start = touch_with(AUDIT, friction=0.3)

    def touch(eng, batch, x):
        got = sub_range_and_warm_start(eng, batch, x)
        M = eng.knots
        if M:                                                                    # and a rollout of the handle's policy, audited where it sits
            gx, gu = _pushed_rollout(eng, x, M, M - 1)
            got += (_audit_dev(eng, x=gx, u=gu, start=1, steps=M - 1).tobytes(),)
        return got

    assert_nothing_else_moves(touch, pac.OPTS)


def test_audit_refusals():
    batch, x, u = assert_common_refusals(AUDIT, pac.OPTS)
    N, B = 6, 2
    eng = DdpEngine("srbd13", N, B, opts=pac.OPTS)
    solve(eng, batch)
    gx, gu = dev(x[:, 1:4]), dev(u[:, 1:3])                                     # rows at the nodes 1 .. 3: start = 1, steps = 2
    assert _audit_dev(eng, x=gx, u=gu, start=1, steps=2).shape == (B, W)
    out = torch.zeros((B, W), dtype=torch.float64, device="cuda")
    vp = eng._dev
    for dx, du in ((vp(gx, gx.shape), None), (None, vp(gu, gu.shape))):         # one of d_x / d_u NULL, whatever start and steps
        with pytest.raises(RuntimeError, match="both NULL"):
            eng._chk(eng.lib.sddp_audit_range_device(eng.h, 0, B, 1, 2, dx, du, 0.0, vp(out, out.shape)))
    big_x = torch.zeros((B, N + 2, eng.nx), dtype=torch.float64, device="cuda")
    big_u = torch.zeros((B, N + 1, eng.nu), dtype=torch.float64, device="cuda")
    for start, steps in ((0, N + 1), (1, N), (N, 1), (-1, 1), (0, 0)):          # (refused before anything is read: the tensors only have to exist)
        with pytest.raises(RuntimeError, match=f"start \\+ steps <= {N}"):
            eng._chk(eng.lib.sddp_audit_range_device(eng.h, 0, B, start, steps, vp(big_x, big_x.shape), vp(big_u, big_u.shape), 0.0, vp(out, out.shape)))
    for start, steps in ((0, N - 1), (1, N - 1), (1, N)):                       # the handle's own plan is audited whole
        with pytest.raises(RuntimeError, match="audited whole"):
            _audit_dev(eng, start=start, steps=steps)
    assert eng.audit().shape == (B, W)                                          # and the handle still works
    eng.close()


def test_fleet_queue_flush_audits_the_solved_range():
    eng, batch, got = assert_fleet_queue_follows_the_last_flush(AUDIT, pac.OPTS)
    x, u, _ = eng.fetch()
    _check("srbd13", omodels.RobotConsts(**batch["consts"]), got[:4], x[:4], u[:4], batch["params"], 0, 0.8, "fleet block 0")
    eng.close()
