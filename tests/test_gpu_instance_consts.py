"""Heterogeneous fleets: per-instance robot constants in one handle (sddp_set_instance_consts, include/sddp.h).

While the table is active every kernel of the handle reads instance b's row of constants.  Checked here: a table that repeats the
handle's constants changes no bit; a heterogeneous batch solves, instance by instance, like the C oracle with that instance's
RobotConsts; the result of an instance does not depend on range, order or slot; model_step / backward / policy export read the
rows too; what cannot differ per instance is refused.  Options as in tests/test_gpu_divergence.py."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle import ddp as oddp, models as omodels
from oracle.cport import stat
from srbd_horizon_amd import workload
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.fleet import FleetQueue
from tests import oracle_refs as refs
from tests.gpu_support import solve as _solve
from tests.variant_cases import SRBD13_FIELDS, TRACKING, draw

pytestmark = pytest.mark.gpu
OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)      # dsrbd_example.py:55-58
SMALL = {"srbd13": (30, 40), "srbd37": (20, 6), "lip30": (20, 6), "srbd61": (20, 4)}      # model -> (N, B) of the bit-equality tests


def _same(got, ref):
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1], ref[1])
    assert got[2].tobytes() == ref[2].tobytes()                  # the raw sddp_stats records


def _oracle(model, csts, batch, opts=None):
    """the C oracle instance by instance, each with its own constants -> (xs, us, stats [B, 8])"""
    out = [refs.c_oracle(model, batch, opts or OPTS, cst=c, sel=[b]) for b, c in enumerate(csts)]
    return tuple(np.concatenate(a) for a in zip(*out))


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wps", [1, 2])
@pytest.mark.parametrize("model", ["srbd13", "srbd37", "lip30", "srbd61"])
def test_a_table_of_the_handles_own_constants_changes_no_bit(model, wps):
    N, B = SMALL[model]
    batch = workload.make_batch(model, N, np.arange(B) + 3)
    eng = DdpEngine(model, N, B, opts=dict(OPTS, waves_per_simd=wps), consts=batch["consts"])
    ref = _solve(eng, batch)
    assert not eng.instance_consts_active()
    eng.set_instance_consts({"m": np.full(B, eng.consts.m)})      # every row: the handle's own constants
    assert eng.instance_consts_active()
    _same(_solve(eng, batch), ref)
    for order in (0, 2):                                          # through a real queue: fewer slots than instances
        q = DdpEngine(model, N, B, opts=dict(OPTS, waves_per_simd=wps, max_slots=max(1, B // 3), queue_order=order), consts=batch["consts"])
        q.set_instance_consts({"m": np.full(B, q.consts.m)})
        _same(_solve(q, batch), ref)
        assert q.queue_info()[1:] == (max(1, B // 3), B)
        q.close()
    eng.clear_instance_consts()
    assert not eng.instance_consts_active()
    _same(_solve(eng, batch), ref)


# ---- 2. / 3. parity of heterogeneous batches with the C oracle, instance by instance ----------------------------------------------
def _parity(model, N, B, fields, long_cap):
    batch = workload.make_batch(model, N, np.arange(B))
    over, csts = draw(batch["consts"], B, fields)
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    eng.set_instance_consts(over)
    x, u, st = _solve(eng, batch)
    xo, uo, so = _oracle(model, csts, batch)
    it_o = stat(so, "iters").astype(int)
    long_ = it_o >= 50                  # long crawls: where GPU and oracle legitimately part
    same = ~long_
    print(f"{model}: oracle iterations mean {it_o.mean():.2f}, {int(long_.sum())} of {B} with >= 50; GPU iterations mean {st['iters'].mean():.2f}; "
          f"iteration counts differ on {np.flatnonzero(st['iters'] != it_o).tolist()}")
    assert long_.sum() <= long_cap
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u)) and np.all(np.isfinite(st["cost"]))
    np.testing.assert_array_equal(st["iters"][same], it_o[same])
    np.testing.assert_array_equal(st["status"][same], stat(so, "status")[same].astype(int))
    np.testing.assert_allclose(st["cost"][same], stat(so, "cost")[same], rtol=1e-8)
    conv = same & (stat(so, "converged") == 1)
    ex, eu = np.max(np.abs(x[conv] - xo[conv])), np.max(np.abs(u[conv] - uo[conv]))
    print(f"{model}: converged {int(conv.sum())}, linf x {ex:.2e} u {eu:.2e}")
    assert ex <= 1e-6 and eu <= 1e-6
    if long_.any():                     # left out of the equality check, not of the test: finite, and no worse than the warm start
        idx = np.flatnonzero(long_)
        sub = {k: batch[k][idx] for k in ("x0", "params", "xs", "us")}
        _, _, s0 = _oracle(model, [csts[i] for i in idx], sub, dict(OPTS, max_iters=0))
        assert np.all(st["cost"][idx] <= stat(s0, "cost"))
    return batch, over, csts, st, it_o


def test_heterogeneous_srbd13_batch_matches_the_oracle_instance_by_instance():
    """B = 256, m, I and four gains drawn per instance.  On the CPU oracle this draw has 11 instances with >= 50 iterations, a mean of
    17.8 iterations, and 200 of 256 instances change their iteration count against the common constants."""
    N, B = 30, 256
    batch, over, csts, st, it_o = _parity("srbd13", N, B, SRBD13_FIELDS, long_cap=(6 * B) // 100)
    s_common = refs.c_oracle("srbd13", batch, OPTS, threads=min(16, os.cpu_count() or 1))[2]
    assert (it_o != stat(s_common, "iters").astype(int)).sum() >= B // 2      # the table matters: ignoring it cannot pass


@pytest.mark.parametrize("model,N,B", [("srbd37", 20, 64), ("lip30", 20, 32), ("srbd61", 20, 32)])
def test_heterogeneous_four_wave_batches_match_the_oracle(model, N, B):
    _parity(model, N, B, TRACKING, long_cap=0)


# ---- 4. range, order and slot independence -------------------------------------------------------------------------------------
def test_heterogeneous_results_do_not_depend_on_range_order_or_slot():
    N, B = 30, 192
    batch = workload.make_batch("srbd13", N, np.arange(B) + 1000)
    over, _ = draw(batch["consts"], B, SRBD13_FIELDS, seed=7)
    one = DdpEngine("srbd13", N, B, opts=OPTS, consts=batch["consts"])
    one.set_instance_consts(over)
    ref = _solve(one, batch)
    assert one.queue_info()[1:] == (B, 0)
    hom = DdpEngine("srbd13", N, B, opts=OPTS, consts=batch["consts"])
    base = _solve(hom, batch)
    assert (ref[2]["iters"] != base[2]["iters"]).sum() > B // 4          # a heterogeneous batch indeed
    # three ranges of one handle
    P = torch.from_numpy(batch["params"]).to("cuda:0")
    torch.cuda.synchronize()
    one.load(batch["x0"], batch["xs"], batch["us"])
    for lo in (0, 64, 128):
        one.solve_range_device(P, lo, 64)
    _same(one.fetch(), ref)
    # few slots, every queue order
    labels, n_cls = workload.srbd13_schedule_classes(batch["params"])
    for order in (0, 2, 3):
        q = DdpEngine("srbd13", N, B, opts=dict(OPTS, max_slots=16, queue_order=order), consts=batch["consts"])
        q.set_instance_consts(over)
        if order == 3:
            q.set_instance_classes(labels, n_cls)
        for _ in range(2):                                                # second solve of order 3: class history exists
            _same(_solve(q, batch), ref)
            assert q.queue_info()[1:] == (16, B)
        q.close()
    # a partial set leaves the other rows alone
    part = DdpEngine("srbd13", N, B, opts=OPTS, consts=batch["consts"])
    part.set_instance_consts({k: v[64:128] for k, v in over.items()}, first=64)
    got = _solve(part, batch)
    for lo, hi, src in ((0, 64, base), (64, 128, ref), (128, B, base)):
        np.testing.assert_array_equal(got[0][lo:hi], src[0][lo:hi])
        np.testing.assert_array_equal(got[1][lo:hi], src[1][lo:hi])
        assert got[2][lo:hi].tobytes() == src[2][lo:hi].tobytes()
    part.set_instance_consts({k: v[:64] for k, v in over.items()})       # a second call keeps the rows of the first
    part.set_instance_consts({k: v[128:] for k, v in over.items()}, first=128)
    _same(_solve(part, batch), ref)


def test_fleet_queue_forwards_the_constants_of_its_shard():
    N, B, D = 30, 32, 2
    batch = workload.make_batch("srbd13", N, np.arange(B) + 40)
    over, _ = draw(batch["consts"], D * B, SRBD13_FIELDS, seed=11)
    t = {k: torch.from_numpy(batch[k]).to("cuda:0") for k in ("x0", "xs", "us", "params")}
    eng = DdpEngine("srbd13", N, D * B, opts=dict(OPTS, max_slots=24, queue_order=2), consts=batch["consts"])
    fleet = FleetQueue(eng, t["params"].repeat(D, 1, 1).contiguous(), B, D)
    fleet.set_instance_consts(over)
    for _ in range(D):
        fleet.submit(t["x0"], t["xs"], t["us"])
    fleet.flush()
    x, u, s = eng.fetch()
    for blk in range(D):
        one = DdpEngine("srbd13", N, B, opts=OPTS, consts=batch["consts"])
        one.set_instance_consts({k: v[blk * B:(blk + 1) * B] for k, v in over.items()})
        ref = _solve(one, batch)
        sl = slice(blk * B, (blk + 1) * B)
        _same((x[sl], u[sl], s[sl]), ref)
    fleet.clear_instance_consts()
    assert not eng.instance_consts_active()


# ---- 5. the other kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["srbd13", "srbd37", "lip30", "srbd61"])
def test_model_step_uses_each_robots_own_dynamics(model):
    N, B = 20, 70                                                        # more than one wavefront of instances
    batch = workload.make_batch(model, N, np.arange(B))
    over, csts = draw(batch["consts"], B, TRACKING, seed=3)
    over["dt"] = np.linspace(0.02, 0.06, B)
    csts = [dataclasses.replace(c, dt=float(d)) for c, d in zip(csts, over["dt"])]
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    eng.set_instance_consts(over)
    rng = np.random.default_rng(5)
    x = batch["x0"] + 0.05 * rng.standard_normal(batch["x0"].shape)
    u = batch["us"][:, 0] + 0.05 * rng.standard_normal(batch["us"][:, 0].shape)
    p = batch["params"][:, 3]
    xn = eng.model_step(x, u, p, 3)
    worst = 0.0
    for b in range(B):
        fo = omodels.make_model(model, csts[b]).f(x[b], u[b], p[b])
        worst = max(worst, float(np.max(np.abs(xn[b] - fo) / np.maximum(np.abs(fo), 1e-300))))
        np.testing.assert_allclose(xn[b], fo, rtol=1e-12, atol=0.0)
    print(f"{model}: model_step worst relative error {worst:.2e}")
    common = omodels.make_model(model, omodels.RobotConsts(**batch["consts"]))
    assert max(np.max(np.abs(xn[b] - common.f(x[b], u[b], p[b]))) for b in range(B)) > 1e-6      # not the handle's robot


@pytest.mark.parametrize("model,N", [("srbd13", 30), ("srbd37", 20)])
def test_backward_sweep_uses_each_robots_own_constants(model, N):
    """Gains of one sweep against oracle.ddp.backward_pass on 8 instances: rtol 1e-7 per entry, with the absolute floor of 1e-8 of
    the largest gain that tests/test_gpu_parity.py gives the same comparison (entries that are structurally zero are rounding
    residues on both sides: a relative bound alone says nothing about them)."""
    B = 8
    batch = workload.make_batch(model, N, np.arange(B) + 20)
    over, csts = draw(batch["consts"], B, TRACKING, seed=9)
    rng = np.random.default_rng(1)
    xs = batch["xs"] + 1e-3 * rng.standard_normal(batch["xs"].shape)
    us = batch["us"] + 1e-3 * rng.standard_normal(batch["us"].shape)
    xs[:, 0] = batch["x0"]
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    eng.set_instance_consts(over)
    eng.load(batch["x0"], xs, us)
    kff, K, scal = eng.backward(batch["params"], mu=0.0)
    xg, ug, Jg = eng.forward(batch["params"], 0.25)
    for b in range(B):
        m = omodels.make_model(model, csts[b])
        P = batch["params"][b]
        d = oddp.defects(m, xs[b], us[b], P)
        ok, Ko, ko, dV1, *_ = oddp.backward_pass(m, xs[b], us[b], P, d, 0.0)
        assert ok and scal[b, 4] == 1.0
        np.testing.assert_allclose(K[b], Ko, rtol=1e-7, atol=1e-8 * max(1.0, np.max(np.abs(Ko))))
        np.testing.assert_allclose(kff[b], ko, rtol=1e-7, atol=1e-8 * max(1.0, np.max(np.abs(ko))))
        assert abs(scal[b, 0] - dV1) <= 1e-8 * max(1.0, abs(dV1))
        xo, uo, Jo = oddp.forward_pass(m, batch["x0"][b], xs[b], us[b], P, d, Ko, ko, 0.25)
        np.testing.assert_allclose(xg[b], xo, rtol=1e-8, atol=1e-8)
        assert abs(Jg[b] - Jo) <= 1e-9 * abs(Jo)


@pytest.mark.parametrize("model,N,B", [("srbd13", 30, 12), ("srbd37", 20, 4)])
def test_policy_of_a_heterogeneous_batch_is_each_robots_own(model, N, B):
    """The policy records of a heterogeneous batch (through a queue) are bit-identical to those of B one-instance homogeneous handles
    built with each robot's constants."""
    batch = workload.make_batch(model, N, np.arange(B) + 60)
    over, _ = draw(batch["consts"], B, TRACKING, seed=13)
    eng = DdpEngine(model, N, B, opts=dict(OPTS, max_slots=3), consts=batch["consts"])
    eng.enable_policy(2)
    eng.set_instance_consts(over)
    x, u, st = _solve(eng, batch)
    eng.policy_range_device()
    rec = eng.fetch_policy()
    assert np.all(rec[:, -1] == 1.0)
    for b in range(B):
        s = slice(b, b + 1)
        consts = dict(batch["consts"], **{k: (v[b] if np.ndim(v[b]) else float(v[b])) for k, v in over.items()})
        one = DdpEngine(model, N, 1, opts=OPTS, consts=consts)
        one.enable_policy(2)
        xb, ub, sb = _solve(one, {k: batch[k][s] for k in ("x0", "xs", "us", "params")})
        one.policy_range_device()
        np.testing.assert_array_equal(xb[0], x[b])
        assert sb.tobytes() == st[s].tobytes()
        np.testing.assert_array_equal(one.fetch_policy()[0], rec[b])
        one.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_what_cannot_differ_per_instance_is_refused_and_the_handle_stays_usable():
    from srbd_horizon_amd import _lib
    N, B = 30, 4
    batch = workload.make_batch("srbd13", N, np.arange(B))
    row = {"m": np.full(B, 41.0)}
    a = np.zeros(19); a[2] = 1.0
    refused = [dict(consts=dict(batch["consts"], extra_rows=[dict(a=a, w=1.0, kind="state")])),      # `_x` build
               dict(consts=dict(batch["consts"], friction_barrier_weight=1e-3)),                     # barrier build
               dict(opts=dict(OPTS, second_order=2))]                                                # second_order = 2 build
    for kw in refused:
        e = DdpEngine("srbd13", N, B, opts=kw.get("opts", OPTS), consts=kw.get("consts", batch["consts"]))
        rows = _lib.pack_instance_consts(_lib.default_consts("srbd13"), row)
        assert e.lib.sddp_set_instance_consts(e.h, 0, B, rows) == -1                                 # SDDP_ERR_ARG
        assert b"plain builds" in e.lib.sddp_last_error(e.h)
        assert not e.instance_consts_active()
        e.close()
    eng = DdpEngine("srbd13", N, B, opts=OPTS, consts=batch["consts"])
    ref = _solve(eng, batch)
    rows = _lib.pack_instance_consts(eng.consts, row)
    for first, count in ((-1, 2), (0, B + 1), (B - 1, 2), (B, 1), (0, 0)):                           # range outside [0, B)
        assert eng.lib.sddp_set_instance_consts(eng.h, first, count, rows) == -1
    for field, val in (("n_extra", 1), ("friction_barrier_weight", 1e-3), ("bound_barrier_weight", 1e-3)):
        bad = _lib.pack_instance_consts(eng.consts, row)
        setattr(bad[2], field, val)
        assert eng.lib.sddp_set_instance_consts(eng.h, 0, B, bad) == -1
    assert eng.lib.sddp_set_instance_consts(eng.h, 0, B, None) == -1
    assert not eng.instance_consts_active()                           # no refused call switched the table on
    with pytest.raises(ValueError):
        eng.set_instance_consts({"friction_barrier_weight": np.zeros(B)})
    with pytest.raises(ValueError):
        eng.set_instance_consts({"no_such_field": np.zeros(B)})
    _same(_solve(eng, batch), ref)                                    # still usable, still homogeneous
    eng.set_instance_consts(row)                                      # and the table still works
    got = _solve(eng, batch)
    assert np.all(np.isfinite(got[0])) and not np.array_equal(got[0], ref[0])
