"""Stationarity certificate on the device (include/sddp.h sddp_stationarity_range_device, sddp_stationarity): record, costates and
reduced gradient of every kernel family, the "_x", the barrier and the second_order = 2 build against the numpy statement of
tests/stationarity_cases.py on the device's own fetched x, u, P.

Tolerances (tests/stationarity_cases.py assert_result; every figure is measured there on the CPU, between the recursion over
oracle.models and over the C port's derivatives, and allowed 64 x on the device):
  * s and word 0: 64 x 2.04e-16 = 1.30e-14 of word 3;   lambda and words 4, 5: 64 x 4.49e-16 = 2.87e-14 of word 5;
  * word 3: 64 x 4.07e-16 of itself;   word 6: 10 x 4.44e-16, absolute (the audit's rule), and bit-equal to the audit's word 10;
  * words 1, 2: the reference's, unless its two largest candidates lie within the tolerance of word 0 of each other (then the reported
    place must hold such a candidate): of the cases only lip30's solved plans, whose whole s is below the tolerance;   word 7 exactly.
The record has no word for the node of the defect, so "word 6 / node against audit words 10 / 11" is checked as word 6 against word 10
and word 7 against the audit's node count (word 12).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import models as omodels
from srbd_horizon_amd import _lib
from srbd_horizon_amd.engine import DdpEngine
from tests import nlp_fixtures as nf, stationarity_cases as sc
from tests.gpu_support import (AUDIT, STATIONARITY, assert_common_refusals, assert_fleet_queue_follows_the_last_flush,
                               assert_nothing_else_moves, solve, solved, touch_with)
from tests.variant_cases import TRACKING, draw

pytestmark = pytest.mark.gpu

W = sc.W


def _run(eng, first=0, count=None, x=None, u=None, full=True):
    """stationarity_device on fresh device tensors -> numpy (record [n, 8], lambda, s), the last two None without `full`"""
    return STATIONARITY.device(eng, first, count, x, u, optional=full)


def _audit(eng, x=None, u=None):
    return AUDIT.device(eng, x=x, u=u)[0]


def _solved(model, N, B, kind):
    return solved(model, N, B, kind, sc.SEEDS[model, kind])


def _check(model, cst, got, x, u, P, label):
    rec, lam, s = got
    m = omodels.make_model(model, cst)
    worst = np.zeros(2)
    for b in range(rec.shape[0]):
        ref = sc.model_reference(m, x[b], u[b], P[b])
        worst = np.maximum(worst, sc.assert_result(rec[b], None if lam is None else lam[b], None if s is None else s[b], ref, label=f"{label} instance {b}"))
    print(f"{label}: worst error / tolerance, s {worst[0]:.3f}, lambda {worst[1]:.3f}")


def _self_consistent(rec, lam, s, audit):
    for b in range(rec.shape[0]):
        assert rec[b, sc.STAT].tobytes() == np.max(np.abs(s[b])).tobytes()
        assert rec[b, sc.LAM0].tobytes() == np.max(np.abs(lam[b, 0])).tobytes()
        assert rec[b, sc.LAM_MAX].tobytes() == np.max(np.abs(lam[b, 1:])).tobytes()
        k, i = int(rec[b, sc.NODE]), int(rec[b, sc.INPUT])
        assert abs(s[b, k, i]) == rec[b, sc.STAT] and np.argmax(np.abs(s[b]).reshape(-1)) == k * s.shape[2] + i      # the first in node-major order
    assert rec[:, sc.DEFECT].tobytes() == audit[:, _lib.AUDIT_DEFECT].tobytes()
    assert rec[:, sc.NODES].tobytes() == audit[:, _lib.AUDIT_NODES].tobytes()


@pytest.mark.parametrize("model,N,B,kind", sc.CASES)
def test_warm_start_and_solved_plan_against_the_reference(model, N, B, kind):
    eng, cst, batch, x, u, st, P = _solved(model, N, B, kind)
    words = C.c_int()
    eng._chk(eng.lib.sddp_stationarity_words(eng.h, C.byref(words)))
    assert words.value == W == 8
    # (a) the warm start, a caller's trajectory
    warm = _run(eng, x=batch["xs"], u=batch["us"])
    _check(model, cst, warm, batch["xs"], batch["us"], P, f"{model} {kind} warm start")
    _self_consistent(*warm, _audit(eng, batch["xs"], batch["us"]))
    # (b) the handle's own solved plan
    own = _run(eng)
    print(f"{model} {kind}: status {st['status']}, word 0 / word 3 of the plan {sc.relative(own[0])}, of the warm start {sc.relative(warm[0])}")
    _check(model, cst, own, x, u, P, f"{model} {kind} plan")
    _self_consistent(*own, _audit(eng))
    host = eng.stationarity()
    assert host.shape == (B, W) and host.dtype == np.float64 and host.tobytes() == own[0].tobytes()
    full = eng.stationarity(full=True)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(full, own))


def test_same_bytes_whatever_the_source_the_range_and_the_optional_outputs():
    eng, cst, batch, x, u, st, P = _solved(*sc.CASES[0])
    B = eng.B
    own = _run(eng)
    same = _run(eng, x=x, u=u)                                                  # the same bytes as a caller's trajectory
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(same, own))
    assert _run(eng, full=False)[0].tobytes() == own[0].tobytes()               # d_lambda / d_grad NULL
    out = torch.full((B, W), 7.0, dtype=torch.float64, device="cuda")
    lam = torch.full((B, eng.N + 1, eng.nx), 7.0, dtype=torch.float64, device="cuda")
    eng.stationarity_device(out, lam=lam)                                       # one of the two
    eng.synchronize()
    assert out.cpu().numpy().tobytes() == own[0].tobytes() and lam.cpu().numpy().tobytes() == own[1].tobytes()
    for first, count in ((1, 3), (4, 1), (0, 2)):
        part = _run(eng, first, count)
        assert all(a.tobytes() == b_[first:first + count].tobytes() for a, b_ in zip(part, own)), (first, count)
        part = _run(eng, first, count, x=x[first:first + count], u=u[first:first + count])      # block i is instance first + i
        assert all(a.tobytes() == b_[first:first + count].tobytes() for a, b_ in zip(part, own)), (first, count)
        assert eng.stationarity(first, count).tobytes() == own[0][first:first + count].tobytes()


def test_nothing_else_moves():
    assert_nothing_else_moves(touch_with(STATIONARITY), sc.OPTS)


def test_instance_constants():
    model, N, B = "srbd13", 6, 5
    eng, cst, batch, x, u, st, P = _solved(*sc.CASES[0])
    own = _run(eng)
    # a table whose rows are all the handle's own robot: the table kernel, the same bytes
    tab = DdpEngine(model, N, B, opts=sc.OPTS, consts=batch["consts"])
    tab.set_instance_consts(dict(m=np.full(B, tab.consts.m)))
    assert tab.instance_consts_active()
    xt, ut, _ = solve(tab, batch)
    assert xt.tobytes() == x.tobytes() and ut.tobytes() == u.tobytes()
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(_run(tab), own))
    tab.close()
    # every robot its own: the record follows each robot's constants, and the handle's own robot misses it
    over, csts = draw(batch["consts"], B, TRACKING, seed=3)
    het = DdpEngine(model, N, B, opts=sc.OPTS, consts=batch["consts"])
    het.set_instance_consts(over)
    xh, uh, _ = solve(het, batch)
    got = _run(het)
    common = omodels.make_model(model, cst)
    for b in range(B):
        _check(model, csts[b], tuple(a[b:b + 1] for a in got), xh[b:b + 1], uh[b:b + 1], P[b:b + 1], f"robot {b}")
        miss = abs(got[0][b, sc.STAT] - sc.model_reference(common, xh[b], uh[b], P[b])[0][sc.STAT]) / got[0][b, sc.SCALE]
        print(f"robot {b}: word 0 / word 3 {sc.relative(got[0][b]):.3e}; the handle's own robot misses word 0 by {miss:.3e} of word 3")
        assert miss > sc.S_TOL
    het.close()


def test_a_nan_stays_on_its_instance():
    eng, cst, batch, x, u, st, P = _solved(*sc.CASES[0])
    own = _run(eng)
    bad = u.copy()
    bad[1, 2, 0] = np.nan                                                       # instance 1, node 2
    got = _run(eng, x=x, u=bad)
    assert np.isnan(got[0][1, sc.STAT]) and got[0][1, sc.NODE] == -1 and got[0][1, sc.INPUT] == -1
    _check("srbd13", cst, got, x, bad, P, "srbd13 with a NaN")
    keep = [0, 2, 3, 4]
    assert all(a[keep].tobytes() == b_[keep].tobytes() for a, b_ in zip(got, own))
    assert not np.isnan(got[1][1, 3:]).any() and np.isnan(got[1][1, 2]).any()   # lambda_3 .. lambda_N do not see node 2
    assert got[0][1, sc.NODES] == eng.N


def test_refusals():
    assert_common_refusals(STATIONARITY, sc.OPTS)


FIXTURES = nf.load_all()


@pytest.mark.parametrize("fx", FIXTURES, ids=[f["name"] for f in FIXTURES])
def test_the_nlp_optima_on_the_device(fx):
    eng = DdpEngine(fx["model"], fx["N"], 1, opts=dict(nf.OPTS, max_iters=0), consts=fx["consts"])
    eng.load(fx["x0"][None], fx["xs0"][None], fx["us0"][None])
    eng.solve(fx["params"][None])
    got = _run(eng, x=fx["x"][None], u=fx["u"][None])
    print(f"{fx['name']}: word 0 / word 3 {sc.relative(got[0][0]):.3e}, word 6 {got[0][0, sc.DEFECT]:.3e}; recorded {sc.FIXTURE_RECORDS[fx['name']][:2]}")
    _check(fx["model"], omodels.RobotConsts(**fx["consts"]), got, fx["x"][None], fx["u"][None], fx["params"][None], fx["name"])
    eng.close()


def test_progress_of_the_solves_that_end_with_status_0():
    """On the status-0 instances of the plain cases for which the C oracle's own solution has word 0 / word 3 below the warm start's
    (tests/test_stationarity_cpu.py: all 13 of 13, none left out), the device's plan has it too."""
    total = taking_part = 0
    for case in sc.PLAIN:
        model, N, B, kind = case
        eng, cst, batch, x, u, st, P = _solved(*case)
        _, _, _, oxs, ous, ost = sc.oracle_plans(*case)
        m = omodels.make_model(model, cst)
        plan, warm = _run(eng, full=False)[0], _run(eng, x=batch["xs"], u=batch["us"], full=False)[0]
        for b in np.flatnonzero(st["status"] == 0):
            total += 1
            if not sc.relative(sc.model_reference(m, oxs[b], ous[b], P[b])[0]) < sc.relative(sc.model_reference(m, batch["xs"][b], batch["us"][b], P[b])[0]):
                continue
            taking_part += 1
            assert sc.relative(plan[b]) < sc.relative(warm[b]), (model, b, sc.relative(plan[b]), sc.relative(warm[b]))
    print(f"{taking_part} of {total} status-0 instances take part")
    assert total > 0 and taking_part >= 0.9 * total


def test_fleet_queue_certifies_the_last_flushed_range():
    assert_fleet_queue_follows_the_last_flush(STATIONARITY, sc.OPTS, "lam")[0].close()
