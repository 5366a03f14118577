"""The three ways a solve gives up -- status 2 (regularisation overflow), 3 (non-finite cost), 4 (line search exhausted, at iteration 0
and after accepted steps) -- on the four PLAIN kernel builds (the builds with traits -- user rows, barriers, second_order = 2, user
builds: tests/test_gpu_failure_exits_builds.py), against the plain-C oracle, and what a failed instance leaves behind: for the
healthy instances that run after it in the same queue slot (the same LDS tiles, dft / rec / gains / candidate buffers) and for the
features behind a solve (resume flag and continue launch, iteration log, class history, policy export, record packing, the
first-knot fetch).  The inputs are the table of tests/failure_cases.py; what the oracle does on each is asserted on the CPU by
tests/test_failure_cases_cpu.py.  Every input passes the library's validation and ends through a documented exit: the bump loop of S2
after one sweep (mu = 2e301 > mu_max), the policy export behind S2 after one more (behind status 3 it makes none), the ladder of S40
after two rungs.

Tolerances: none of its own.  A failed record (parity.assert_failed_matches_c_oracle): status, iters, converged, alpha and (S2, S3)
rollouts = 0 exact; mu rel 1e-12; cost and gap rel 1e-9 where the oracle's are finite, non-finite exactly where they are not; the
returned trajectory the start's bytes with row 0 = x0 (S2, S3a..d, S40), the oracle's iterate at 1e-6 (S4 mid-solve), the oracle's
non-finite mask and 1e-6 on the finite entries (S3e).  A healthy instance of a mixed batch: parity.assert_matches_c_oracle, and the
bytes of the same handle configuration on the all-healthy twin.  Everything behind the solve is an exact comparison.

Measured on an MI355X (profiles/failure_exits/README.md has the table): 171 tests in 13 s.  Failed records, 47 ids: every exact
field exact; S2, S3a..d and S40 return the start byte for byte, cost within 6.5e-16 and gap within 2.9e-15 where finite; the mid-solve
iterates within l-inf x 8.7e-9, u 1.5e-10, cost 2.2e-10, gap 1.2e-15 (bounds 1e-6, 1e-6, 1e-9, 1e-9); S3e x 3.7e-15 on the finite
entries.  Containment: 41 ids x 9 handle configurations, 1539 healthy instances byte-identical to the all-healthy batch.  A mid-solve
status 4 exists for srbd13 and srbd61, none for srbd37 and lip30 (tests/failure_cases.py).  Two bugs found and fixed: the policy export
behind status 3 (four-wavefront models: ok = 1, NaN gains) and sddp_apply_policy_device on an ok = 0 record whose x_0 holds a NaN.
Deliberate breaks on scratch builds (README): the sweep's upper pivot bound dropped fails every S2 id of that kernel family and
nothing else; the resume flag as status != 0 fails the resume test on S2, S3 and S4; the policy rows not zeroed fails the policy
tests; the copy-back skipped at status 4 fails the mid-solve ids only.

test_status_3_from_a_nan_start[srbd13] is the former tests/test_gpu_api.py::test_non_finite_start_is_reported_not_propagated (its
input is case S3a; what it asserted is asserted here on every failing and healthy instance, on all four models).
"""
import numpy as np
import pytest
import torch

from oracle import ddp as oddp, models as omodels
from srbd_horizon_amd import _lib, dist as sdist, workload
from srbd_horizon_amd.engine import DdpEngine
from tests import failure_cases as fc, options_cases as oc, parity, policy_cases as pc
from tests.gpu_support import BUILDS, same_bytes, snap, solve as _solve

pytestmark = pytest.mark.gpu

F = {f: i for i, f in enumerate(_lib.LOG_FIELDS)}
ALL = [(n, w) for n, c in fc.CASES.items() for w in BUILDS[c.model]]
CONTAINED = [(n, w) for n in fc.MIXED for w in BUILDS[fc.CASES[n].model]]               # every mixed batch: NaN keys (S3a, S3c), inf keys (S3b, S3d)
CONFIGS = [(0, 0)] + [(slots, order) for slots in (1, 2) for order in (0, 1, 2, 3)]          # (max_slots, queue_order)
PLAIN = {m: BUILDS[m][0] for m in fc.MODELS}


def _engine(c, s, wps, **over):
    return DdpEngine(c.model, c.N, len(c.seeds), opts=dict(fc.options(c), waves_per_simd=wps, **over), consts=s["consts"])


def _start_of(c, s, b):
    """the trajectory a failed instance returns, where it is the start (row 0 = x0); None: the oracle's iterate"""
    return None if c.kind in ("S3e", "S4m") else (s["x0"][b], s["xs"][b], s["us"][b])


def _check_against_oracle(name, x, u, st):
    c, s = fc.CASES[name], fc.start(name)
    xo, uo, so = fc.oracle(name)
    for b in c.fail:
        parity.assert_failed_matches_c_oracle(x, u, st, xo, uo, so, b, start=_start_of(c, s, b), rollouts=0 if c.kind[1] in "23" else None)
    h = fc.healthy_idx(c)
    if len(h):
        # S40's healthy instances restart at the oracle's optimum: their own defects are rounding of f, at most 8 eps |x| per entry
        slack = c.N * x.shape[2] * 8 * np.finfo(float).eps * np.max(np.abs(xo[h]), axis=(1, 2)) if c.kind == "S40" else 0.0
        parity.assert_matches_c_oracle(x[h], u[h], st[h], xo[h], uo[h], so[h], gap_slack=slack)
    return parity.failed_deviations(x, u, st, xo, uo, so, c.fail)


@pytest.mark.parametrize("name,wps", ALL)
def test_failed_record_matches_the_c_oracle(name, wps):
    c, s = fc.CASES[name], fc.start(name)
    eng = _engine(c, s, wps)
    x, u, st = _solve(eng, s)
    conv = eng.is_converged()
    eng.close()
    print(f"{name} w{wps}: status {st['status'].tolist()} iters {st['iters'].tolist()} rollouts {st['rollouts'].tolist()}")
    d = _check_against_oracle(name, x, u, st)
    print(f"{name} w{wps}: failing instances, finite entries: {parity.summary(d)}")
    np.testing.assert_array_equal(conv, st["status"] == 0)
    if c.kind == "S2":
        assert (st["mu"] == 10.0 * fc.MU0_S2 + oddp.DdpOptions().mu_min).all() and (st["rollouts"] == 0).all()


@pytest.mark.parametrize("model", fc.MODELS)
def test_status_3_from_a_nan_start(model):
    """a NaN in x0 and in the x warm start of some instances: they end with status 3, not converged, no iteration; the others are
    unaffected (status 0, converged).  Default options, as a caller who sets none."""
    name = f"S3a-{model}"
    c, s = fc.CASES[name], fc.start(name)
    eng = DdpEngine(model, c.N, len(c.seeds), consts=s["consts"])
    eng.load(s["x0"], s["xs"], s["us"])
    eng.solve(s["params"])
    st = eng.stats.copy()
    eng.close()
    for b in range(len(c.seeds)):
        if b in c.fail:
            assert st["status"][b] == 3 and st["converged"][b] == 0 and st["iters"][b] == 0, (b, st[b])
        else:
            assert st["status"][b] == 0 and st["converged"][b] == 1, (b, st[b])


def _apply_at_x0(eng, x, u):
    """sddp_apply_policy_device with x_meas = x_0 -> u_out [B, nu].  The tensors are made on torch's stream and used on the handle's:
    torch finishes first."""
    dev = torch.device("cuda", 0)
    out = torch.full((x.shape[0], u.shape[2]), 7.0, dtype=torch.float64, device=dev)
    x_meas = torch.from_numpy(x[:, 0].copy()).to(dev)
    torch.cuda.synchronize()
    eng.apply_policy_device(x_meas, out)
    eng.synchronize()
    return out.cpu().numpy()


def _labels(c, s):
    return workload.schedule_classes(c.model, s["params"])


@pytest.mark.parametrize("name,wps", CONTAINED)
def test_failed_instances_stay_contained(name, wps):
    """the mixed batch against its all-healthy twin under the same handle configuration: every healthy instance holds the same
    bytes.  max_slots = 1 runs the whole batch through one slot: every healthy instance right behind a failed one."""
    c, s, t = fc.CASES[name], fc.start(name), fc.healthy(name)
    B, h = len(c.seeds), fc.healthy_idx(c)
    compared = 0
    for slots, order in CONFIGS:
        res = []
        for batch in (s, t):
            eng = _engine(c, batch, wps, max_slots=slots, queue_order=order)
            if order == 3:
                eng.set_instance_classes(*_labels(c, batch))
            out = _solve(eng, batch)
            if order == 1:                                                # again: the history of the first launch orders the second
                out = _solve(eng, batch)
            if slots and order:                                           # an ordered queue: the order holds NaN and inf keys
                assert sorted(eng.last_queue_order()[:B].tolist()) == list(range(B)), (slots, order)
            eng.close()
            res.append(out)
        same_bytes(res[0], res[1], h, msg=f"({name} w{wps} max_slots {slots} queue_order {order})")
        assert (res[1][2]["status"] == 0).all()
        _check_against_oracle(name, *res[0])
        compared += len(h)
    print(f"{name} w{wps}: {compared} healthy instances byte-identical to the all-healthy batch over {len(CONFIGS)} configurations")


@pytest.mark.parametrize("model,wps", [(m, w) for m in fc.MODELS for w in BUILDS[m]])
@pytest.mark.parametrize("order", [0, 2])
def test_status_2_followed_by_the_next_instance_in_the_same_slot(model, wps, order):
    """max_slots = 1: the whole S2 batch through one slot, every instance right behind a failed sweep (on the four-wavefront kernel the
    only exit taken with the aliased tiles half-written); each record against the oracle, the start returned byte for byte"""
    name = f"S2-{model}"
    c, s = fc.CASES[name], fc.start(name)
    eng = _engine(c, s, wps, max_slots=1, queue_order=order)
    x, u, st = _solve(eng, s)
    assert eng.queue_info()[1:] == (1, len(c.seeds))
    if order:
        assert sorted(eng.last_queue_order()[:len(c.seeds)].tolist()) == list(range(len(c.seeds)))
    eng.close()
    _check_against_oracle(name, x, u, st)
    assert (st["rollouts"] == 0).all()


# ---- behind the solve ----------------------------------------------------------------------------------------------------------------
RESUME = [(f"S3c-{m}", 2) for m in fc.MODELS] + [(f"S2-{m}", 2) for m in fc.MODELS] + [("S4m-srbd13", 3), ("S4m-srbd61", 2), ("S40-srbd37", 2)]


@pytest.mark.parametrize("name,k", RESUME)
def test_resume_flag_and_continue_launch(name, k):
    c, s = fc.CASES[name], fc.start(name)
    B = len(c.seeds)
    full = _engine(c, s, PLAIN[c.model])
    full.enable_resume()
    uncut = _solve(full, s)
    full.close()
    eng = _engine(c, s, PLAIN[c.model], max_iters=k)
    eng.enable_resume()
    cut = _solve(eng, s)
    status = cut[2]["status"]
    gave_up = np.isin(status, (2, 3, 4))
    assert gave_up[[b for b in c.fail if uncut[2]["iters"][b] < k]].all()
    assert eng.unfinished() == int((status == 1).sum())
    for b in range(B):
        assert eng.unfinished(b, 1) == int(status[b] == 1), (b, status[b])       # the flag, instance by instance
    eng.set_options(max_iters=fc.BASE["max_iters"])
    eng.continue_solve()
    done = snap(eng)
    same_bytes(done, cut, np.flatnonzero(gave_up), msg=f"({name}: failed instances after the continue launch)")
    same_bytes(done, uncut, msg=f"({name}: continued against uncut)")
    assert eng.unfinished() == 0
    eng.close()
    print(f"{name}: cut at {k}: status {status.tolist()}; continued to {done[2]['status'].tolist()}")


@pytest.mark.parametrize("name", [f"{k}-{m}" for m in fc.MODELS for k in ("S2", "S3c", "S3e", "S40")] + list(fc.MID))
def test_iteration_log_of_a_failed_instance(name):
    c, s = fc.CASES[name], fc.start(name)
    eng = _engine(c, s, PLAIN[c.model])
    eng.enable_resume()
    eng.enable_iteration_log(32)
    x, u, st = _solve(eng, s)
    rec, n = eng.iteration_log()
    eng.close()
    tried = fc.S40_TRIED if c.kind == "S40" else fc.MID_TRIED.get(name)
    for b in c.fail:
        if c.kind[1] in "23":
            assert n[b] == 0, (b, n[b])
            continue
        o = fc.oracle_trace(name, b)
        g = rec[b, :n[b]]
        assert n[b] == len(o) > st["iters"][b], (b, n[b], len(o))
        for f in ("alpha", "theta", "tried"):
            np.testing.assert_array_equal(g[:, F[f]], [r[f] for r in o], err_msg=f"instance {b} {f}")
        np.testing.assert_array_equal(g[:, F["iters"]], np.cumsum([r["alpha"] > 0.0 for r in o]), err_msg=f"instance {b} iters")
        last = g[-1]
        assert last[F["alpha"]] == 0.0 and last[F["J_accepted"]] == 0.0 and last[F["tried"]] == tried and last[F["iters"]] == st["iters"][b]
        assert last[F["J"]].tobytes() == st["cost"][b].tobytes() and last[F["rollouts"]] == st["rollouts"][b]
        for f, tol in (("J", parity.COST_RTOL), ("gap", parity.GAP_RTOL)):
            ref = np.array([r[f] for r in o])
            assert (np.abs(g[:, F[f]] - ref) <= tol * np.abs(ref)).all(), (b, f, g[:, F[f]], ref)
    print(f"{name}: records per instance {n.tolist()}")


@pytest.mark.parametrize("name", [f"S3c-{m}" for m in fc.MODELS] + ["S2-srbd13", "S2-srbd37", "S40-srbd37"] + list(fc.MID))
def test_class_history_counts_a_failed_instance_once(name):
    c, s = fc.CASES[name], fc.start(name)
    labels, n_classes = _labels(c, s)
    eng = _engine(c, s, PLAIN[c.model], max_slots=2, queue_order=3)
    eng.set_instance_classes(labels, n_classes)
    x, u, st = _solve(eng, s)
    got = eng.class_stats()
    want = np.zeros((n_classes, 2), dtype=np.uint64)
    np.add.at(want[:, 0], labels, st["iters"].astype(np.uint64))
    np.add.at(want[:, 1], labels, np.uint64(1))
    np.testing.assert_array_equal(got, want)
    assert int(got[:, 1].sum()) == len(c.seeds)
    for cl in np.unique(labels):
        m, k = eng.class_history(int(cl))
        assert k == int((labels == cl).sum()) and abs(m - st["iters"][labels == cl].mean()) <= 1e-12
    eng.close()
    _check_against_oracle(name, x, u, st)


@pytest.mark.parametrize("model", fc.MODELS)
def test_policy_export_behind_status_2(model):
    name, M = f"S2-{model}", 3
    c, s = fc.CASES[name], fc.start(name)
    eng = _engine(c, s, PLAIN[model], mu0=0.0)
    eng.enable_policy(M)
    _solve(eng, s)                                                        # a healthy solve first: its gains fill the policy rows,
    eng.policy_range_device()                                             # so zeros behind the failed one are zeros that were written
    kff, K, info = eng.policy()
    assert (info[:, 3] == 1.0).all() and kff.any(axis=(1, 2)).all() and K.any(axis=(1, 2, 3)).all()
    eng.set_options(mu0=fc.MU0_S2)
    x, u, st = _solve(eng, s)
    assert (st["status"] == 2).all()
    eng.policy_range_device()
    kff, K, info = eng.policy()
    opt = oddp.DdpOptions(**fc.options(c))
    tail = np.array([10.0 * (10.0 * fc.MU0_S2 + opt.mu_min) + opt.mu_min, 0.0, 0.0, 0.0])
    for b in range(len(c.seeds)):
        assert info[b].tobytes() == tail.tobytes(), (b, info[b])
    assert not kff.any() and not K.any()                                  # exactly 0 (no -0.0 either: any() is False for it, so look at bytes)
    assert kff.tobytes() == np.zeros_like(kff).tobytes() and K.tobytes() == np.zeros_like(K).tobytes()
    m = omodels.make_model(model, fc.consts(name))
    ko, Ko, io = pc.oracle_policy(m, x[0], u[0], s["params"][0], st[0], opt, M)          # the rule, with the bounded backward_pass
    assert io.tobytes() == tail.tobytes() and not ko.any() and not Ko.any()
    assert _apply_at_x0(eng, x, u).tobytes() == np.ascontiguousarray(u[:, 0]).tobytes()      # ok = 0, x_meas = x_0: u_0 exactly
    eng.close()


@pytest.mark.parametrize("model", fc.MODELS)
@pytest.mark.parametrize("kind", ["S3a", "S3c"])
def test_policy_export_behind_status_3(model, kind):
    """an iterate the solve refused for its non-finite cost has no policy: ok = 0, zeros, mu_used = the solve's mu, no sweep.  (Before
    this rule the four-wavefront models, whose Quu does not depend on u, passed the sweep behind S3c and exported (0, 0, NaN, 1) with
    NaN gains; srbd13 bumped mu past mu_max.)  Healthy neighbours: the bytes of the all-healthy batch's policies."""
    name, M = f"{kind}-{model}", 3
    c, s, t = fc.CASES[name], fc.start(name), fc.healthy(name)
    h = fc.healthy_idx(c)
    opt = oddp.DdpOptions(**fc.options(c))
    m = omodels.make_model(model, fc.consts(name))
    eng = _engine(c, s, PLAIN[model])
    eng.enable_policy(M)
    _solve(eng, t)                                                        # the all-healthy batch first, on the same handle: its gains
    eng.policy_range_device()                                             # fill every policy row the failed instances must zero
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
        assert got[b].tobytes() == np.ascontiguousarray(u[b, 0]).tobytes(), b      # ok = 0, x_meas = x_0: u_0 exactly (bytes: NaNs too)
    assert (info[h, 3] == 1.0).all()
    assert mixed[h].tobytes() == twin[h].tobytes()                        # the healthy neighbours' policies


@pytest.mark.parametrize("model", fc.MODELS)
@pytest.mark.parametrize("kind", ["S3c", "S3b", "S2"])
def test_packed_records_and_first_knot_fetch_of_failed_instances(model, kind):
    """sddp_pack_records_device against dist.pack_records_into on the fetched results, bit for bit (NaN and inf included), and
    sddp_solve_resident_first against the stats.  The output tensor is filled on torch's stream and packed on the handle's: torch
    finishes first (without that the fill can land behind the pack: seen once, as the fill value in the middle of a record)."""
    name = f"{kind}-{model}"
    c, s = fc.CASES[name], fc.start(name)
    B = len(c.seeds)
    eng = _engine(c, s, PLAIN[model])
    x, u, st = _solve(eng, s)
    dev = torch.device("cuda", 0)
    for mode in ("full", "first_knot"):
        W = eng.record_words(mode)
        out = torch.full((B, W), 7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
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


@pytest.mark.parametrize("status", [2, 3, 4])
def test_ddpsolver_returns_false_for_each_failure_exit(status):
    """the drop-in surface: DDPSolver.solve() is False and sddp_is_converged 0 for a solve that gave up (srbd13)"""
    from srbd_horizon_amd.ddp import DDPSolver
    b = workload.make_batch("srbd13", 30, [0])                            # instance 0 of the table's srbd13 batches, through the solver
    over = {2: fc.S2_OVER, 3: {}, 4: fc.S40_OVER}[status]
    solver = DDPSolver(b["problem"].prb, opts=dict(fc.BASE, **over))
    x0, xs = b["x0"][0].copy(), b["xs"][0].copy()
    if status == 3:
        x0[3:7] = np.nan
        xs[:, 3:7] = np.nan
    solver.setInitialState(x0)
    solver.set_x_warmstart(xs.T)
    solver.set_u_warmstart(b["us"][0].T)
    assert solver.solve() is False
    assert solver.stats["status"] == status and solver.stats["converged"] == 0 and solver.stats["iters"] == 0
    assert not solver.ddp_solver.is_converged().any()
