"""The failure exits -- status 2, 3 (from a NaN, from an inf in a widened parameter column, from an exponential barrier that overflows
on finite inputs) and 4 (at iteration 0 and after accepted steps) -- on the kernel builds WITH traits: the `_x` builds (user rows), the
barrier builds (friction cone, bounds), the second_order = 2 builds, both together, and a generated user build.
tests/test_gpu_failure_exits.py covers the plain builds; this module repeats its checks on the table of tests/failure_build_cases.py,
whose behaviour on the oracles tests/test_failure_build_cases_cpu.py asserts without a GPU.  Also here: healthy solves in which a
line-search candidate's barrier overflows in the middle of a ladder (Lc): the rung must be rejected and the next one tried.

Tolerances: none of its own.  A failed record: parity.assert_failed_matches_c_oracle (exact status, iters, converged, alpha, rollouts =
0 behind S2 and S3; the start's bytes behind S2, S3* and S40; the oracle's iterate at 1e-6 behind S4b).  A healthy instance:
parity.assert_matches_c_oracle with the S40 gap slack of tests/test_gpu_failure_exits.py; on the user build, whose reference is the
numpy oracle with the user rows (one build, no rho), parity.assert_matches_numpy_oracle.  Everything else is a comparison of bytes
(gpu_support.same_bytes).

second_order = 2: the build and its larger derivative record are chosen at create and not visible in any result; what a caller can
see of them is that the handle refuses to leave the build (sddp_set_options with second_order = 1: "another kernel build and record
size"), which the test asserts before and after the failed batch.

Lc: builds with traits have no iteration-log variant, so the ladder is checked through stats.rollouts, which must equal the count that
failure_build_cases.expected_rollouts derives from the oracle's trace (a kernel that accepted the overflowed rung, or skipped rungs
behind it, takes another number of passes), and through sddp_debug_poison_lds, which must not change a byte.

Measured figures, the searches behind S4b and Lc and the deliberate breaks: profiles/failure_exits/README.md.
"""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import cport, ddp as oddp, models as omodels
from srbd_horizon_amd import dist as sdist, workload
from srbd_horizon_amd.engine import DdpEngine
from tests import failure_build_cases as fb, parity, policy_cases as pc, user_terms_defs as ud
from tests.gpu_support import BUILDS, same_bytes, solve as _solve

pytestmark = pytest.mark.gpu

ALL = [(n, w) for n in fb.FAILING for w in BUILDS[fb.CASES[n].model]]
CONTAINED = [(n, w) for n in fb.MIXED for w in BUILDS[fb.CASES[n].model]]
CONFIGS = [(0, 0), (1, 0), (1, 2), (2, 3)]                                 # (max_slots, queue_order)
PAIRS = [(b, m) for b, models in fb.BUILDS.items() for m in models]
BEHIND = [f"{k}-{b}-{m}" for b, m in PAIRS for k in ("S3c", "S2")]          # one mixed S3 case and the S2 case of each build
NO_POLICY = ("friction", "bound", "so2", "so2-friction")


@functools.lru_cache(maxsize=None)
def _user_build(N):
    return ud.user_case(fb.USER_CASE, N)[1]


def _engine(c, s, wps=None, **over):
    opts = dict(fb.options(c), waves_per_simd=BUILDS[c.model][0] if wps is None else wps, **over)
    return DdpEngine(c.model, c.N, len(c.seeds), opts=opts, consts=s["consts"], model_id=_user_build(c.N) if c.build == "user" else None)


def _start_of(c, s, b):
    return None if c.kind == "S4b" else (s["x0"][b], s["xs"][b], s["us"][b])


def _check_against_oracle(name, x, u, st):
    c, s = fb.CASES[name], fb.start(name)
    xo, uo, so = fb.oracle(name)
    for b in c.fail:
        parity.assert_failed_matches_c_oracle(x, u, st, xo, uo, so, b, start=_start_of(c, s, b), rollouts=0 if c.kind[1] in "23" else None)
    h = fb.healthy_idx(c)
    if len(h) and c.build == "user":
        for b in h:
            r = types.SimpleNamespace(xs=xo[b], us=uo[b], iters=int(cport.stat(so, "iters")[b]), cost=cport.stat(so, "cost")[b])
            parity.assert_matches_numpy_oracle(x[b], u[b], st[b], r, b)
            assert st["status"][b] == 0 and st["converged"][b] == 1, (b, st[b])
    elif len(h):
        # S40's healthy instances restart at the oracle's optimum: their own defects are rounding of f, at most 8 eps |x| per entry
        slack = c.N * x.shape[2] * 8 * np.finfo(float).eps * np.max(np.abs(xo[h]), axis=(1, 2)) if c.kind == "S40" else 0.0
        parity.assert_matches_c_oracle(x[h], u[h], st[h], xo[h], uo[h], so[h], gap_slack=slack)
    return parity.failed_deviations(x, u, st, xo, uo, so, c.fail)


def _stays_on_the_so2_build(eng):
    with pytest.raises(RuntimeError, match="another kernel build and record size"):
        eng.set_options(second_order=1)
    eng.opts.second_order = 2


@pytest.mark.parametrize("name,wps", ALL)
def test_failed_record_matches_the_oracle(name, wps):
    c, s = fb.CASES[name], fb.start(name)
    eng = _engine(c, s, wps)
    if c.build in fb.SO2:
        _stays_on_the_so2_build(eng)
    x, u, st = _solve(eng, s)
    conv = eng.is_converged()
    if c.build in fb.SO2:
        _stays_on_the_so2_build(eng)
    eng.close()
    print(f"{name} w{wps}: status {st['status'].tolist()} iters {st['iters'].tolist()} rollouts {st['rollouts'].tolist()}")
    d = _check_against_oracle(name, x, u, st)
    print(f"{name} w{wps}: failing instances, finite entries: {parity.summary(d)}")
    np.testing.assert_array_equal(conv, st["status"] == 0)
    if c.kind == "S2":
        assert (st["mu"] == 10.0 * fb.fc.MU0_S2 + oddp.DdpOptions().mu_min).all() and (st["rollouts"] == 0).all()


def _labels(c, s):
    return workload.schedule_classes(c.model, s["params"][:, :, :fb.base_columns(c.model)])      # the base parameter columns


@pytest.mark.parametrize("name,wps", CONTAINED)
def test_failed_instances_stay_contained(name, wps):
    """the mixed batch against its all-healthy twin under the same handle configuration: every healthy instance holds the same
    bytes.  max_slots = 1 runs the whole batch through one slot: every healthy instance right behind a failed one."""
    c, s, t = fb.CASES[name], fb.start(name), fb.healthy(name)
    B, h = len(c.seeds), fb.healthy_idx(c)
    for slots, order in CONFIGS:
        res = []
        for batch in (s, t):
            eng = _engine(c, batch, wps, max_slots=slots, queue_order=order)
            if order == 3:
                eng.set_instance_classes(*_labels(c, batch))
            out = _solve(eng, batch)
            if slots and order:                                           # an ordered queue: the order holds NaN and inf keys
                assert sorted(eng.last_queue_order()[:B].tolist()) == list(range(B)), (slots, order)
            eng.close()
            res.append(out)
        same_bytes(res[0], res[1], h, msg=f"({name} w{wps} max_slots {slots} queue_order {order})")
        assert (res[1][2]["status"] == 0).all()
        _check_against_oracle(name, *res[0])


@pytest.mark.parametrize("build,model,wps", [(b, m, w) for b, m in PAIRS for w in BUILDS[m]])
@pytest.mark.parametrize("order", [0, 2])
def test_status_2_followed_by_the_next_instance_in_the_same_slot(build, model, wps, order):
    name = f"S2-{build}-{model}"
    c, s = fb.CASES[name], fb.start(name)
    eng = _engine(c, s, wps, max_slots=1, queue_order=order)
    x, u, st = _solve(eng, s)
    assert eng.queue_info()[1:] == (1, len(c.seeds))
    if order:
        assert sorted(eng.last_queue_order()[:len(c.seeds)].tolist()) == list(range(len(c.seeds)))
    eng.close()
    _check_against_oracle(name, x, u, st)
    assert (st["rollouts"] == 0).all()


@pytest.mark.parametrize("name,wps", [(n, w) for n in fb.LC for w in BUILDS[fb.CASES[n].model]])
def test_an_overflowed_candidate_is_rejected_and_the_next_rung_tried(name, wps):
    c, s = fb.CASES[name], fb.start(name)
    xo, uo, so = fb.oracle(name)
    want = np.array([fb.expected_rollouts(c.model, fb.oracle_trace(name, b)) for b in range(len(c.seeds))])
    eng = _engine(c, s, wps)
    x, u, st = _solve(eng, s)
    print(f"{name} w{wps}: iters {st['iters'].tolist()} rollouts {st['rollouts'].tolist()} oracle's ladders {want.tolist()}; "
          f"{parity.summary(parity.deviations(x, u, st, xo, uo, so))}")
    parity.assert_matches_c_oracle(x, u, st, xo, uo, so)
    np.testing.assert_array_equal(st["rollouts"], want)
    eng.poison_lds()                                                      # nothing of an overflowed candidate is read by the next rung
    same_bytes(_solve(eng, s), (x, u, st), msg=f"({name} w{wps}: after sddp_debug_poison_lds)")
    eng.close()


# ---- behind the solve ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BEHIND)
def test_packed_records_first_knot_fetch_and_class_history(name):
    """sddp_pack_records_device (both modes) against dist.pack_records_into on the fetched results, bit for bit, and
    sddp_solve_resident_first against the stats, on failed and healthy instances; the class history counts a failed instance once"""
    c, s = fb.CASES[name], fb.start(name)
    B = len(c.seeds)
    labels, n_classes = _labels(c, s)
    eng = _engine(c, s, max_slots=2, queue_order=3)
    eng.set_instance_classes(labels, n_classes)
    x, u, st = _solve(eng, s)
    got = eng.class_stats()
    want = np.zeros((n_classes, 2), dtype=np.uint64)
    np.add.at(want[:, 0], labels, st["iters"].astype(np.uint64))
    np.add.at(want[:, 1], labels, np.uint64(1))
    np.testing.assert_array_equal(got, want)
    assert int(got[:, 1].sum()) == B
    dev = torch.device("cuda", 0)
    for mode in ("full", "first_knot"):
        W = eng.record_words(mode)
        out = torch.full((B, W), 7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()                                          # the fill is on torch's stream, the pack on the handle's
        eng.pack_records_device(out, 0, B, mode)
        eng.synchronize()
        ref = torch.empty((B, W), dtype=torch.float64)
        sdist.pack_records_into(ref, torch.from_numpy(x), torch.from_numpy(u), torch.from_numpy(st["cost"].copy()), torch.from_numpy(st["iters"].copy()), mode)
        assert out.cpu().numpy().tobytes() == ref.numpy().tobytes(), mode
    eng.load(s["x0"], s["xs"], s["us"])
    eng.set_params(s["params"])
    u0, x1 = eng.solve_resident_first()
    fs = eng.first_stats
    np.testing.assert_array_equal(fs["status"], st["status"])
    np.testing.assert_array_equal(fs["iters"], st["iters"])
    assert fs["cost"].tobytes() == st["cost"].tobytes()
    assert u0.tobytes() == np.ascontiguousarray(u[:, 0]).tobytes() and x1.tobytes() == np.ascontiguousarray(x[:, 1]).tobytes()
    eng.close()
    _check_against_oracle(name, x, u, st)


def _apply_at_x0(eng, x, u):
    dev = torch.device("cuda", 0)
    out = torch.full((x.shape[0], u.shape[2]), 7.0, dtype=torch.float64, device=dev)
    x_meas = torch.from_numpy(x[:, 0].copy()).to(dev)
    torch.cuda.synchronize()
    eng.apply_policy_device(x_meas, out)
    eng.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("model", fb.BUILDS["x"])
def test_policy_export_behind_status_2_on_the_x_builds(model):
    name, M = f"S2-x-{model}", 3
    c, s = fb.CASES[name], fb.start(name)
    eng = _engine(c, s, mu0=0.0)
    eng.enable_policy(M)
    _solve(eng, s)                                                        # a healthy solve first: its gains fill the policy rows
    eng.policy_range_device()
    kff, K, info = eng.policy()
    assert (info[:, 3] == 1.0).all() and kff.any(axis=(1, 2)).all() and K.any(axis=(1, 2, 3)).all()
    eng.set_options(mu0=fb.fc.MU0_S2)
    x, u, st = _solve(eng, s)
    assert (st["status"] == 2).all()
    eng.policy_range_device()
    kff, K, info = eng.policy()
    opt = oddp.DdpOptions(**fb.options(c))
    tail = np.array([10.0 * (10.0 * fb.fc.MU0_S2 + opt.mu_min) + opt.mu_min, 0.0, 0.0, 0.0])
    for b in range(len(c.seeds)):
        assert info[b].tobytes() == tail.tobytes(), (b, info[b])
    assert kff.tobytes() == np.zeros_like(kff).tobytes() and K.tobytes() == np.zeros_like(K).tobytes()
    m = omodels.make_model(model, fb.refs.consts(s))
    ko, Ko, io = pc.oracle_policy(m, x[0], u[0], s["params"][0], st[0], opt, M)
    assert io.tobytes() == tail.tobytes() and not ko.any() and not Ko.any()
    assert _apply_at_x0(eng, x, u).tobytes() == np.ascontiguousarray(u[:, 0]).tobytes()
    eng.close()


@pytest.mark.parametrize("model", fb.BUILDS["x"])
@pytest.mark.parametrize("kind", ["S3c", "S3x"])
def test_policy_export_behind_status_3_on_the_x_builds(model, kind):
    """ok = 0, zeros, mu_used = the solve's mu behind a refused iterate -- also where the non-finite entry sits in a widened
    parameter column; the healthy neighbours: the bytes of the all-healthy batch's policies"""
    name, M = f"{kind}-x-{model}", 3
    c, s, t = fb.CASES[name], fb.start(name), fb.healthy(name)
    h = fb.healthy_idx(c)
    opt = oddp.DdpOptions(**fb.options(c))
    m = omodels.make_model(model, fb.refs.consts(s))
    eng = _engine(c, s)
    eng.enable_policy(M)
    _solve(eng, t)
    eng.policy_range_device()
    twin = eng.fetch_policy()
    assert (twin[:, -1] == 1.0).all() and twin[:, :-4].any(axis=1).all()
    x, u, st = _solve(eng, s)
    eng.policy_range_device()
    mixed = eng.fetch_policy()
    kff, K, info = eng.split_policy(mixed)
    got = _apply_at_x0(eng, x, u)
    eng.close()
    for b in c.fail:
        assert st["status"][b] == 3
        ko, Ko, io = pc.oracle_policy(m, x[b], u[b], s["params"][b], st[b], opt, M)
        assert info[b].tobytes() == io.tobytes() == np.array([st["mu"][b], 0.0, 0.0, 0.0]).tobytes(), (b, info[b], io)
        assert kff[b].tobytes() == ko.tobytes() == np.zeros_like(ko).tobytes() and K[b].tobytes() == Ko.tobytes() == np.zeros_like(Ko).tobytes(), b
        assert got[b].tobytes() == np.ascontiguousarray(u[b, 0]).tobytes(), b
    assert (info[h, 3] == 1.0).all()
    assert mixed[h].tobytes() == twin[h].tobytes()


@pytest.mark.parametrize("build,model", PAIRS)
def test_refusals_leave_the_handle_usable_after_a_failed_batch(build, model):
    """behind a mixed batch: sddp_enable_resume is refused on every build with traits, sddp_enable_policy on the barrier and
    second_order = 2 builds, in their existing words; the same handle then solves the all-healthy twin to a fresh handle's bytes"""
    name = f"S3c-{build}-{model}"
    c, s, t = fb.CASES[name], fb.start(name), fb.healthy(name)
    fresh = _engine(c, t)
    ref = _solve(fresh, t)
    fresh.close()
    eng = _engine(c, s)
    x, u, st = _solve(eng, s)
    with pytest.raises(RuntimeError, match="sddp_enable_resume: resumable solves exist for the plain builds only"):
        eng.enable_resume()
    eng.resume_enabled = False
    if build in NO_POLICY:
        with pytest.raises(RuntimeError, match="sddp_enable_policy: no policy kernel for this build"):
            eng.enable_policy(3)
    _check_against_oracle(name, x, u, st)
    same_bytes(_solve(eng, t), ref, msg=f"({name}: the twin on the handle that refused)")
    assert (ref[2]["status"] == 0).all()
    eng.close()
