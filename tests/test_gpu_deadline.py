"""Time-budgeted launches (include/sddp.h sddp_set_time_budget): a launch cut at a device-clock deadline is a max_iters cut.

Every claim reduces to a byte identity against kernels that exist without the budget: an instance cut by the clock after k accepted
iterations holds the bytes of an ordinary handle's solve at max_iters = k, and continued to the end it is the uncut solve.  Shapes,
inputs and slot counts are those of tests/resume_cases.py; every comparison is `==` on the raw bytes of xs, us and the sddp_stats
records (tests/gpu_support.py same_bytes).

TINY is one tick of the 100 MHz clock: the deadline has always passed by the time an instance reaches its first test, so what the
launch does is decided by min_iters alone and is deterministic.  The cut in the middle (test 4) is the one test whose cut points the
clock decides; it checks every instance against the reference for the iteration count it was cut at, whatever that is."""
import numpy as np
import pytest
import torch

from tests import resume_cases as rc
from tests.gpu_support import continue_to, cut_ref, log_engine, log_of, logged, resume_engine, same_bytes, snap, uncut, used_rows
from tests.gpu_support import cut as cut_at
from tests.resume_cases import IDENTITY
from tests.variant_cases import SRBD13_FIELDS, draw

pytestmark = pytest.mark.gpu

TINY = 0.01          # microseconds: round(100 * 0.01) = 1 clock tick
NEVER = 60e6         # 60 s
BUILDS = [("srbd13", 1), ("srbd13", 2), ("srbd37", 1), ("srbd37", 2), ("lip30", 2), ("srbd61", 1)]
KS = {m: sorted({0, 1, rc.CUT[m]}) for m in rc.SHAPES}      # lip30: {0, 1}


def _budgeted(eng, b, budget_us, min_iters, total=rc.TOTAL):
    """a fresh solve of the whole batch at max_iters = total under the budget"""
    eng.set_time_budget(budget_us, min_iters)
    return cut_at(eng, b, total)


# ---- 1. a deadline that never arrives ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,case,wps", IDENTITY)
def test_a_budget_that_never_runs_out_changes_nothing(model, case, wps):
    """Nothing is cut by time: unfinished() counts no instance but those the uncut solve itself leaves at the cap (status 1 with
    iters == max_iters; 4 of the 48 single-shooting srbd13 instances run into max_iters = 100, every other case has none)."""
    ref = uncut(model, case, wps)
    eng = resume_engine(model, case, wps)
    got = _budgeted(eng, rc.batch(model), NEVER, 0)
    assert eng.time_budget() == (NEVER, 0)
    same_bytes(got, ref)
    capped = (ref[2]["status"] == 1) & (ref[2]["iters"] == rc.TOTAL)
    assert eng.unfinished() == int(capped.sum()) == int((ref[2]["status"] == 1).sum())
    if (model, case) != ("srbd13", "ir1"):
        assert eng.unfinished() == 0
    eng.close()


# ---- 2. expired on arrival: min_iters decides, and the cut is the max_iters cut ------------------------------------------------
@pytest.mark.parametrize("model,wps", BUILDS)
def test_expired_on_arrival_is_the_cut_at_min_iters(model, wps):
    b = rc.batch(model)
    eng = resume_engine(model, "base", wps)
    for k in KS[model]:
        got = _budgeted(eng, b, TINY, k)
        same_bytes(got, cut_ref(model, wps, k), msg=f"(min_iters {k})")
        n_open = int((got[2]["status"] == 1).sum())
        assert eng.unfinished() == n_open and n_open >= 1
        assert (got[2]["iters"][got[2]["status"] == 1] == k).all()
        start, deadline = eng.deadline_clock()
        assert deadline - start == 1 and eng.deadline_overrun_us() > 0.0
    eng.set_time_budget(2.5, 0)
    cut_at(eng, b, 0)
    start, deadline = eng.deadline_clock()
    assert deadline - start == 250                              # round(100 * budget_us) ticks of the 100 MHz clock
    eng.close()


# ---- 3. then continued ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,wps", BUILDS)
def test_a_time_cut_continued_is_the_uncut_solve_and_min_iters_is_per_launch(model, wps):
    b, ref = rc.batch(model), uncut(model, "base", wps)
    eng = resume_engine(model, "base", wps)
    for k in KS[model]:
        _budgeted(eng, b, TINY, k)
        eng.set_time_budget(0.0)
        assert eng.time_budget() == (0.0, 0)
        same_bytes(continue_to(eng, rc.TOTAL), ref, msg=f"(cut by time at {k}, continued)")
        assert eng.unfinished() == 0
    # every continue launch under the expired budget owes its instances one iteration more: 1 + 3 launches = max_iters 4
    first = 1
    _budgeted(eng, b, TINY, first)
    eng.set_time_budget(TINY, 1)
    for _ in range(3):
        got = continue_to(eng, rc.TOTAL)
    same_bytes(got, cut_ref(model, wps, first + 3), msg="(three continue launches of one iteration each)")
    eng.set_time_budget(0.0)
    same_bytes(continue_to(eng, rc.TOTAL), ref, msg="(cut by time four times, continued)")
    eng.close()


# ---- 4. cut in the middle: the clock decides where ------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["srbd13", "srbd37"])
def test_a_cut_in_the_middle_leaves_every_instance_at_a_max_iters_cut(model):
    """srbd37: the four-wave kernel's workgroup-uniform decision.  The budget is a quarter of the launch's own kernel time on a queue
    several instances deep per slot (srbd13: 12, srbd37: 4), so most of the work is undone when it runs out."""
    wps = 2
    b, ref = rc.batch(model), uncut(model, "base", wps)
    eng = resume_engine(model, "base", wps, queue_order=0)
    eng.enable_timing()
    for _ in range(2):                                           # the second launch: code and clocks are warm
        same_bytes(cut_at(eng, b, rc.TOTAL), ref)
        T_ms = eng.last_kernel_ms()
    budget_us = 1e3 * T_ms / 4.0
    got = _budgeted(eng, b, budget_us, 0)
    overrun = eng.deadline_overrun_us()
    st = got[2]
    cut = st["status"] == 1
    print(f"{model} w{wps}: uncut launch {1e3 * T_ms:.1f} us, budget {budget_us:.1f} us, cut {int(cut.sum())} of {len(st)} at iterations "
          f"{st['iters'][cut].tolist()} (uncut {ref[2]['iters'][cut].tolist()}), overrun {overrun:.1f} us")
    assert cut.any(), "nothing was cut: the test would pass empty"
    assert eng.unfinished() == int(cut.sum())
    same_bytes(got, ref, sel=~cut, msg="(finished inside the budget)")
    assert (st["iters"][cut] <= ref[2]["iters"][cut]).all()
    for k in sorted(set(st["iters"][cut].tolist())):
        same_bytes(got, cut_ref(model, wps, int(k)), sel=cut & (st["iters"] == k), msg=f"(cut by the clock at {k})")
    eng.set_time_budget(0.0)
    same_bytes(continue_to(eng, rc.TOTAL), ref, msg="(cut in the middle, continued)")
    eng.close()


# ---- 5. with the iteration log ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,wps", [("srbd13", 2), ("srbd37", 2)])
def test_the_log_of_a_time_cut_and_continued_solve_is_the_uncut_log(model, wps):
    b, ref = rc.batch(model), logged(model, "base", wps)
    eng = log_engine(model, "base", wps)
    cut_at(eng, b, rc.CUT[model])
    log_k = log_of(eng)
    eng.set_time_budget(TINY, rc.CUT[model])
    at_cut = cut_at(eng, b, rc.TOTAL)
    log_cut = log_of(eng)
    assert (at_cut[2]["status"] == 1).any()
    assert (log_cut[1] == log_k[1]).all() and used_rows(*log_cut) == used_rows(*log_k)      # the records of the max_iters cut
    eng.set_time_budget(0.0)
    eng.set_options(max_iters=rc.TOTAL)
    eng.continue_solve()
    done = snap(eng)
    lg = log_of(eng)
    eng.close()
    assert done[2].tobytes() == ref[2].tobytes() and done[0].tobytes() == ref[0].tobytes() and done[1].tobytes() == ref[1].tobytes()
    assert (lg[1] == ref[4]).all() and used_rows(*lg) == used_rows(ref[3], ref[4])


# ---- 6. with an instance-constants table -------------------------------------------------------------------------------------------
def test_a_heterogeneous_batch_is_cut_by_time_with_each_robots_own_constants():
    model, wps = "srbd13", 2
    b, (N, B) = rc.batch(model), rc.SHAPES[model]
    over, _ = draw(b["consts"], B, SRBD13_FIELDS, seed=7)
    plain = resume_engine(model, "base", wps, resume=False)
    plain.set_instance_consts(over)
    eng = resume_engine(model, "base", wps)
    eng.set_instance_consts(over)
    total = cut_at(plain, b, rc.TOTAL)
    assert (total[2]["iters"] != uncut(model, "base", wps)[2]["iters"]).any()      # a heterogeneous batch indeed
    refs = {k: cut_at(plain, b, k) for k in KS[model] + [4]}
    for k in KS[model]:
        got = _budgeted(eng, b, TINY, k)
        same_bytes(got, refs[k], msg=f"(table, min_iters {k})")
        assert eng.unfinished() == int((got[2]["status"] == 1).sum()) >= 1
        eng.set_time_budget(0.0)
        same_bytes(continue_to(eng, rc.TOTAL), total, msg=f"(table, cut by time at {k}, continued)")
    _budgeted(eng, b, TINY, 1)
    eng.set_time_budget(TINY, 1)
    for _ in range(3):
        got = continue_to(eng, rc.TOTAL)
    same_bytes(got, refs[4], msg="(table, three continue launches of one iteration each)")
    plain.close(); eng.close()


# ---- 7. class history ----------------------------------------------------------------------------------------------------------------
def test_class_history_does_not_count_an_instance_cut_by_time():
    model = "srbd13"
    b, ref, B = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model][1]
    labels = (np.arange(B) % 3).astype(np.int32)
    eng = resume_engine(model, "base", 2, queue_order=3)
    eng.set_instance_classes(labels, 3)
    at_cut = _budgeted(eng, b, TINY, rc.CUT[model])
    open_ = at_cut[2]["status"] == 1
    assert open_.any() and (~open_).any()
    for c in range(3):
        mean, n = eng.class_history(c)
        sel = (labels == c) & ~open_
        assert n == sel.sum() and mean * n == pytest.approx(at_cut[2]["iters"][sel].sum())
    eng.set_time_budget(0.0)
    same_bytes(continue_to(eng, rc.TOTAL), ref)
    for c in range(3):
        mean, n = eng.class_history(c)
        sel = labels == c
        assert n == sel.sum() and mean * n == pytest.approx(ref[2]["iters"][sel].sum())
    eng.close()


# ---- 8. refusals: the handle stays usable --------------------------------------------------------------------------------------------
def test_the_budget_is_refused_where_it_cannot_work():
    model = "srbd13"
    b, ref = rc.batch(model), uncut(model, "base", 1)
    eng = resume_engine(model, "base", resume=False)
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        eng.set_time_budget(100.0)
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        eng.device_buffer(11)
    assert eng.time_budget() == (0.0, 0)
    same_bytes(cut_at(eng, b, rc.TOTAL), ref)
    eng.enable_resume()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="budget_us"):
            eng.set_time_budget(bad)
    with pytest.raises(RuntimeError, match="min_iters"):
        eng.set_time_budget(100.0, -1)
    assert eng.time_budget() == (0.0, 0)
    assert eng.device_buffer(11)[1] == 16
    same_bytes(cut_at(eng, b, rc.TOTAL), ref)
    eng.set_time_budget(TINY, 2)                                 # sddp_enable_resume(h, 0) disarms it
    eng.enable_resume(False)
    assert eng.time_budget() == (0.0, 0)
    eng.enable_resume()
    assert eng.time_budget() == (0.0, 0)
    same_bytes(cut_at(eng, b, rc.TOTAL), ref)
    eng.close()
    for kw in (dict(consts=dict(b["consts"], friction_barrier_weight=1e-3)), dict(second_order=2)):
        eng = resume_engine(model, "base", resume=False, **kw)
        with pytest.raises(RuntimeError, match="plain builds only"):
            eng.enable_resume()
        with pytest.raises(RuntimeError, match="sddp_enable_resume"):
            eng.set_time_budget(100.0)
        got = cut_at(eng, b, rc.TOTAL)
        assert (got[2]["status"] != 1).all() and np.isfinite(got[2]["cost"]).all()
        eng.close()


# ---- 9. the Python layers ------------------------------------------------------------------------------------------------------------
def test_fleet_queue_solve_within_returns_the_records_of_solve_sliced():
    from srbd_horizon_amd.fleet import FleetQueue
    model = "srbd13"
    b, ref, (N, B) = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    out = []
    for how in ("within", "sliced"):
        eng = resume_engine(model, "base", 2, resume=False)
        q = FleetQueue(eng, dev(b["params"]), B, 1)
        q.submit(dev(b["x0"]), dev(b["xs"]), dev(b["us"]))
        finished, records = q.solve_within(TINY, rc.TOTAL) if how == "within" else q.solve_sliced(rc.CUT[model], rc.TOTAL)
        torch.cuda.synchronize()
        same_bytes(snap(eng), ref)
        assert q.launches == 2
        assert not eng.resume_enabled and eng.opts.max_iters == rc.TOTAL      # the engine is left as it was found
        with pytest.raises(RuntimeError, match="sddp_enable_resume"):
            eng.unfinished()
        out.append((finished.cpu().numpy(), records.cpu().numpy(), q))
        eng.close()
    assert out[0][1].tobytes() == out[1][1].tobytes()
    assert not out[0][0].any()                                   # expired on arrival, min_iters = 0: nobody finished inside it
    assert out[0][2].overrun_us > 0.0


def test_mpc_loop_under_a_budget_that_never_runs_out_visits_the_states_of_the_plain_loop():
    from srbd_horizon_amd.mpc import EXAMPLE_OPTS, MpcLoop
    states = []
    for budget in (None, NEVER):
        loop = MpcLoop("srbd13", ns=10, opts=dict(EXAMPLE_OPTS, max_iters=100), budget_us=budget)
        seq = []
        for _ in range(12):
            loop.tick("walking", (1.0, 0.0))
            seq.append(loop.state.copy())
        assert loop.solver.ddp_solver.resume_enabled == (budget is not None)
        if budget is not None:
            assert loop.solver.ddp_solver.time_budget() == (NEVER, 1)
        states.append(np.array(seq))
    assert (states[0] == states[1]).all()
