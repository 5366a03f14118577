"""Resumable solves (include/sddp.h): a solve cut at max_iters = k and continued is the uncut solve, byte for byte.

The inputs and cut points are those of tests/resume_cases.py, whose kinds of carried state (open gaps, closed gaps with theta = 1,
a bumped mu, converged before the cut) tests/test_resume_cpu.py asserts on the C oracle.  Every comparison between GPU results is
`==` on the raw bytes of xs, us and the sddp_stats records (iters and rollouts included): the continued solve performs the same
operations on the same bits, there is nothing to tolerate.  Only the comparison with the C oracle (test 7) has tolerances, the ones
tests/test_gpu_options.py applies to the same kind of comparison.

srbd13 runs 48 instances on max_slots = 4: slots are reused within a launch and differ between the launches, so a carry row
indexed by slot fails tests 1, 3, 4 and 6."""
import functools

import numpy as np
import pytest
import torch

from srbd_horizon_amd import workload
from srbd_horizon_amd.engine import DdpEngine
from tests import options_cases as oc, resume_cases as rc

pytestmark = pytest.mark.gpu

IDENTITY = [("srbd13", "base", 1), ("srbd13", "base", 2), ("srbd13", "ir1", 2), ("srbd13", "so0", 1), ("srbd13", "A", 2), ("srbd13", "E", 1),
            ("srbd37", "base", 1), ("srbd37", "base", 2), ("srbd37", "ir1", 2), ("srbd37", "so0", 1), ("srbd37", "E", 2),
            ("lip30", "base", 2), ("lip30", "ir1", 2), ("srbd61", "base", 1), ("srbd61", "ir1", 1)]


def _engine(model, case, wps=1, resume=True, consts=None, **over):
    N, B = rc.SHAPES[model]
    opts = dict(rc.options(case), waves_per_simd=wps, max_slots=rc.MAX_SLOTS[model])
    opts.update(over)
    eng = DdpEngine(model, N, B, opts=opts, consts=rc.batch(model)["consts"] if consts is None else consts)
    if resume:
        eng.enable_resume()
    return eng


def _load(eng, b):
    eng.set_initial_state(b["x0"]); eng.set_x_warmstart(b["xs"]); eng.set_u_warmstart(b["us"])


def _snap(eng):
    x, u, st = eng.fetch()
    return x.copy(), u.copy(), st.copy()


def _cut(eng, b, k):
    """a fresh solve of the whole batch with max_iters = k (through sddp_solve: the parameters become the resident tensor)"""
    eng.set_options(max_iters=k)
    _load(eng, b)
    eng.solve(b["params"])
    return _snap(eng)


def _continue(eng, k, first=0, count=None):
    eng.set_options(max_iters=k)
    eng.continue_solve(None, first, count)
    return _snap(eng)


def _same(got, ref, sel=slice(None), msg=""):
    assert got[0][sel].tobytes() == ref[0][sel].tobytes(), f"xs differ {msg}"
    assert got[1][sel].tobytes() == ref[1][sel].tobytes(), f"us differ {msg}"
    if got[2][sel].tobytes() != ref[2][sel].tobytes():
        for f in ref[2].dtype.names:
            np.testing.assert_array_equal(got[2][f][sel], ref[2][f][sel], err_msg=f"stats.{f} {msg}")
        raise AssertionError(f"stats differ in their padding {msg}")


@functools.lru_cache(maxsize=None)
def uncut(model, case, wps):
    """the ordinary handle (no sddp_enable_resume) at max_iters = 100: computed once, read-only"""
    eng = _engine(model, case, wps, resume=False)
    out = _cut(eng, rc.batch(model), rc.TOTAL)
    eng.close()
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. bit identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,case,wps", IDENTITY)
def test_cut_and_continued_is_the_uncut_solve_byte_for_byte(model, case, wps):
    b, ref = rc.batch(model), uncut(model, case, wps)
    eng = _engine(model, case, wps)
    at_cut = _cut(eng, b, rc.CUT[model])
    n_cut = int((at_cut[2]["status"] == 1).sum())
    two = _continue(eng, rc.TOTAL)
    k1, k2 = rc.CUTS3[model]
    _cut(eng, b, k1)
    _continue(eng, k2)
    three = _continue(eng, rc.TOTAL)
    eng.close()
    print(f"{model} {case} w{wps}: uncut iterations {ref[2]['iters'].tolist()}, unfinished at {rc.CUT[model]}: {n_cut}")
    assert n_cut >= 1                                            # the cut did cut something
    if model == "srbd13" and case == "base":
        assert n_cut < rc.SHAPES[model][1]                       # ... and left finished instances beside them
    _same(two, ref, msg="(cut, continued)")
    _same(three, ref, msg="(cut, continued, continued)")


# ---- 2. the cut itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,wps", [("srbd13", 1), ("srbd13", 2), ("srbd37", 2), ("srbd61", 1)])
def test_the_cut_of_a_resumable_handle_is_the_cut_of_an_ordinary_one(model, wps):
    b = rc.batch(model)
    plain, res = _engine(model, "base", wps, resume=False), _engine(model, "base", wps)
    _same(_cut(res, b, rc.CUT[model]), _cut(plain, b, rc.CUT[model]))
    res.enable_resume(False)                                     # and back on the ordinary kernels
    _same(_cut(res, b, rc.TOTAL), uncut(model, "base", wps))
    plain.close(); res.close()


# ---- 3. finished instances are left alone; the count ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["srbd13", "srbd37"])
def test_a_continue_launch_leaves_finished_instances_alone(model):
    b = rc.batch(model)
    eng = _engine(model, "base", 2)
    assert eng.unfinished() == 0                                 # never solved
    at_cut = _cut(eng, b, rc.CUT[model])
    open_ = at_cut[2]["status"] == 1
    assert eng.unfinished() == int(open_.sum()) and 0 < open_.sum()
    lo = rc.SHAPES[model][1] // 4
    assert eng.unfinished(lo, 2 * lo) == int(open_[lo:3 * lo].sum())
    done = _continue(eng, rc.TOTAL)
    _same(done, at_cut, sel=~open_, msg="(instances with flag 0)")
    _same(done, uncut(model, "base", 2))
    assert (done[2]["status"] != 1).all() and eng.unfinished() == 0
    again = _continue(eng, rc.TOTAL)                             # nothing left to continue: nothing changes
    _same(again, done)
    eng.close()


# ---- 4. ranges and order -------------------------------------------------------------------------------------------------------------
def test_a_range_continues_its_instances_only():
    model = "srbd13"
    b, ref, B = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model][1]
    eng = _engine(model, "base", 2)
    at_cut = _cut(eng, b, rc.CUT[model])
    lo, n = 8, 16
    got = _continue(eng, rc.TOTAL, lo, n)
    inside = np.zeros(B, dtype=bool); inside[lo:lo + n] = True
    assert (at_cut[2]["status"][inside] == 1).any() and (at_cut[2]["status"][~inside] == 1).any()
    _same(got, at_cut, sel=~inside, msg="(outside the range)")
    _same(got, ref, sel=inside, msg="(inside the range)")
    eng.close()


@pytest.mark.parametrize("order", [0, 1, 2])
def test_two_halves_in_either_order_under_every_queue_order(order):
    model = "srbd13"
    b, ref, B = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model][1]
    eng = _engine(model, "base", 2, queue_order=order)
    for halves in (((0, B // 2), (B // 2, B // 2)), ((B // 2, B // 2), (0, B // 2))):
        _cut(eng, b, rc.CUT[model])
        eng.set_options(max_iters=rc.TOTAL)
        for lo, n in halves:
            eng.continue_solve(None, lo, n)
            assert eng.queue_info()[1:] == (rc.MAX_SLOTS[model], n)          # a queue on few slots
        _same(_snap(eng), ref, msg=f"(queue_order {order}, halves {halves})")
    eng.close()


# ---- 5. invalidation and errors -----------------------------------------------------------------------------------------------------
def test_rewritten_instances_cannot_be_continued():
    model = "srbd13"
    b, ref, (N, B) = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model]
    eng = _engine(model, "base", 2)
    at_cut = _cut(eng, b, rc.CUT[model])
    open_ = at_cut[2]["status"] == 1
    lo, n = 4, 20
    assert open_[lo:lo + n].any() and open_[lo + n:].any()
    x0 = torch.from_numpy(b["x0"][lo:lo + n].copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.load_range_device(lo, n, x0=x0)                          # the same values: xs / us / stats keep their bytes
    touched = np.zeros(B, dtype=bool); touched[lo:lo + n] = True
    assert eng.unfinished() == int((open_ & ~touched).sum())
    got = _continue(eng, rc.TOTAL)
    _same(got, at_cut, sel=touched, msg="(sddp_load_range_device: invalidated)")
    _same(got, ref, sel=~touched, msg="(the others)")
    # sddp_advance rewrites every instance
    eng.set_options(max_iters=rc.CUT[model])
    _load(eng, b); eng.set_params(b["params"]); eng.solve_resident()
    assert eng.unfinished() == int(open_.sum())
    eng.advance(b["params"][:, -1], b["x0"])
    assert eng.unfinished() == 0
    before = _snap(eng)
    _same(_continue(eng, rc.TOTAL), before, msg="(sddp_advance: invalidated)")
    eng.close()


def test_continue_is_refused_where_it_cannot_work():
    model = "srbd13"
    b = rc.batch(model)
    eng = _engine(model, "base", resume=False)
    _cut(eng, b, rc.CUT[model])
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        eng.continue_solve()
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        eng.unfinished()
    eng.close()
    eng = _engine(model, "base")
    _load(eng, b)
    with pytest.raises(RuntimeError, match="no solve has run|no resident parameters"):
        eng.continue_solve()
    P = torch.from_numpy(b["params"].copy()).to("cuda:0")
    with pytest.raises(RuntimeError, match="no solve has run"):
        eng.continue_solve(P)
    _same(_cut(eng, b, rc.TOTAL), uncut(model, "base", 1))       # the handle stays usable
    eng.close()
    for kw in (dict(consts=dict(b["consts"], friction_barrier_weight=1e-3)), dict(second_order=2)):
        eng = _engine(model, "base", resume=False, **kw)
        with pytest.raises(RuntimeError, match="plain builds only"):
            eng.enable_resume()
        _cut(eng, b, rc.CUT[model])
        with pytest.raises(RuntimeError, match="sddp_enable_resume"):
            eng.continue_solve()
        eng.close()
    # lip30 has one build and takes second_order = 2 through sddp_set_options: not together with resumable solves, either way round
    lip = _engine("lip30", "base", 2)
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        lip.set_options(second_order=2)
    lip.opts.second_order = 1
    lip.enable_resume(False)
    lip.set_options(second_order=2)
    with pytest.raises(RuntimeError, match="plain builds only"):
        lip.enable_resume()
    lip.close()


# ---- 6. with an instance-constants table -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["srbd13", "srbd37"])
def test_a_heterogeneous_batch_is_continued_with_each_robots_own_constants(model):
    from tests.test_gpu_instance_consts import SRBD13_FIELDS, TRACKING, draw
    b, (N, B) = rc.batch(model), rc.SHAPES[model]
    over, _ = draw(b["consts"], B, SRBD13_FIELDS if model == "srbd13" else TRACKING, seed=7)
    plain = _engine(model, "base", 2, resume=False)
    plain.set_instance_consts(over)
    ref = _cut(plain, b, rc.TOTAL)
    assert (ref[2]["iters"] != uncut(model, "base", 2)[2]["iters"]).any()      # a heterogeneous batch indeed
    eng = _engine(model, "base", 2)
    eng.set_instance_consts(over)                                # (clears the flags: before the cut)
    at_cut = _cut(eng, b, rc.CUT[model])
    assert (at_cut[2]["status"] == 1).any()
    _same(_continue(eng, rc.TOTAL), ref)
    plain.close(); eng.close()


# ---- 7. against the oracle -------------------------------------------------------------------------------------------------------------
def test_the_continued_solve_agrees_with_the_c_oracle():
    """tolerances: tests/test_gpu_options.py test_case_matches_the_c_oracle (iters, status, converged, alpha exact; mu rel 1e-12; l-inf of
    x and u 1e-6; cost and gap rel 1e-9; rho RHO_RTOL).  Pins that the two halves together still agree with the oracle, not the path."""
    from tests.test_gpu_options import RHO_RTOL
    model = "srbd13"
    b = rc.batch(model)
    eng = _engine(model, "base", 2)
    _cut(eng, b, rc.CUT[model])
    x, u, st = _continue(eng, rc.TOTAL)
    eng.close()
    xo, uo, so = rc.oracle(model, "base")
    np.testing.assert_array_equal(st["iters"], oc.stat(so, "iters").astype(int))
    np.testing.assert_array_equal(st["status"], oc.stat(so, "status").astype(int))
    np.testing.assert_array_equal(st["converged"], oc.stat(so, "converged").astype(int))
    np.testing.assert_array_equal(st["alpha"], oc.stat(so, "alpha"))
    for i in range(len(st)):
        assert st["mu"][i] == pytest.approx(so[i, 5], rel=1e-12)
        assert np.max(np.abs(x[i] - xo[i])) <= 1e-6 and np.max(np.abs(u[i] - uo[i])) <= 1e-6, i
        assert abs(st["cost"][i] - so[i, 0]) <= 1e-9 * abs(so[i, 0]), i
        assert abs(st["gap"][i] - so[i, 4]) <= 1e-9 * abs(so[i, 4]), i
        assert abs(st["rho"][i] - so[i, 7]) <= RHO_RTOL * abs(so[i, 7]), i


# ---- 8. policy behind a continue ---------------------------------------------------------------------------------------------------
def test_the_policy_behind_the_last_slice_is_the_policy_behind_the_uncut_solve():
    model = "srbd13"
    b = rc.batch(model)
    plain, eng = _engine(model, "base", 2, resume=False), _engine(model, "base", 2)
    recs = []
    for e, cuts in ((plain, ()), (eng, (rc.CUT[model],))):
        e.enable_policy(1)
        _cut(e, b, cuts[0] if cuts else rc.TOTAL)
        if cuts:
            _continue(e, rc.TOTAL)
        e.policy_range_device()
        recs.append(e.fetch_policy().copy())
        e.close()
    assert (recs[0][:, -1] == 1.0).all()                         # ok
    assert recs[1].tobytes() == recs[0].tobytes()


# ---- 9. MpcLoop in slices -------------------------------------------------------------------------------------------------------------
def test_mpc_loop_in_slices_visits_the_states_of_the_uncut_loop():
    from srbd_horizon_amd.mpc import EXAMPLE_OPTS, MpcLoop
    states, conts = [], 0
    for slices in (None, (2, 100)):
        loop = MpcLoop("srbd13", ns=10, opts=dict(EXAMPLE_OPTS, max_iters=100), slices=slices)
        seq = []
        for _ in range(12):
            loop.tick("walking", (1.0, 0.0))
            seq.append(loop.state.copy())
            if slices and loop.solver.stats["iters"] > slices[0]:
                conts += 1
        states.append(np.array(seq))
    assert conts >= 1                                            # some tick did need its second slice
    assert (states[0] == states[1]).all()


# ---- class history: counted once, by the launch that finishes the instance ---------------------------------------------------------
def test_class_history_counts_an_instance_once_with_its_total_iterations():
    model = "srbd13"
    b, ref, B = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model][1]
    labels = (np.arange(B) % 3).astype(np.int32)
    eng = _engine(model, "base", 2, queue_order=3)
    eng.set_instance_classes(labels, 3)
    at_cut = _cut(eng, b, rc.CUT[model])
    open_ = at_cut[2]["status"] == 1
    for c in range(3):
        mean, n = eng.class_history(c)
        sel = (labels == c) & ~open_
        assert n == sel.sum() and mean * n == pytest.approx(at_cut[2]["iters"][sel].sum())
    _same(_continue(eng, rc.TOTAL), ref)
    for c in range(3):
        mean, n = eng.class_history(c)
        sel = labels == c
        assert n == sel.sum() and mean * n == pytest.approx(ref[2]["iters"][sel].sum())
    eng.close()


# ---- FleetQueue.solve_sliced ------------------------------------------------------------------------------------------------------
def test_fleet_queue_solve_sliced_returns_the_uncut_records():
    from srbd_horizon_amd.fleet import FleetQueue
    model = "srbd13"
    b, ref, (N, B) = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    eng = _engine(model, "base", 2, resume=False)
    q = FleetQueue(eng, dev(b["params"]), B, 1)
    q.submit(dev(b["x0"]), dev(b["xs"]), dev(b["us"]))
    finished, records = q.solve_sliced(rc.CUT[model], rc.TOTAL)
    torch.cuda.synchronize()
    _same(_snap(eng), ref)
    fin, rec, first = finished.cpu().numpy(), records.cpu().numpy(), q.first_records.cpu().numpy()
    assert 0 < fin.sum() < B and q.launches == 2
    want = np.concatenate([ref[1][:, 0], ref[0][:, 1], ref[2]["cost"][:, None], ref[2]["iters"][:, None].astype(float)], axis=1)
    assert rec.tobytes() == want.tobytes()
    assert first[fin].tobytes() == want[fin].tobytes()           # what the first slice handed out was final
    assert not eng.resume_enabled and eng.opts.max_iters == rc.TOTAL      # the engine is left as it was found
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        eng.unfinished()
    eng.close()
