"""Resumable solves (include/sddp.h): a solve cut at max_iters = k and continued is the uncut solve, byte for byte.

The inputs and cut points are those of tests/resume_cases.py, whose kinds of carried state (open gaps, closed gaps with theta = 1,
a bumped mu, converged before the cut) tests/test_resume_cpu.py asserts on the C oracle.  Every comparison between GPU results is
`==` on the raw bytes of xs, us and the sddp_stats records (iters and rollouts included): the continued solve performs the same
operations on the same bits, there is nothing to tolerate.  Only the comparison with the C oracle (test 7) has tolerances, those of
tests/parity.py.

srbd13 runs 48 instances on max_slots = 4: slots are reused within a launch and differ between the launches, so a carry row
indexed by slot fails tests 1, 3, 4 and 6."""
import numpy as np
import pytest
import torch

from tests import parity, resume_cases as rc
from tests.gpu_support import continue_to, cut, resume_engine, same_bytes, snap, uncut
from tests.variant_cases import SRBD13_FIELDS, TRACKING, draw
from tests.resume_cases import IDENTITY

pytestmark = pytest.mark.gpu

# ---- 1. bit identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,case,wps", IDENTITY)
def test_cut_and_continued_is_the_uncut_solve_byte_for_byte(model, case, wps):
    b, ref = rc.batch(model), uncut(model, case, wps)
    eng = resume_engine(model, case, wps)
    at_cut = cut(eng, b, rc.CUT[model])
    n_cut = int((at_cut[2]["status"] == 1).sum())
    two = continue_to(eng, rc.TOTAL)
    k1, k2 = rc.CUTS3[model]
    cut(eng, b, k1)
    continue_to(eng, k2)
    three = continue_to(eng, rc.TOTAL)
    eng.close()
    print(f"{model} {case} w{wps}: uncut iterations {ref[2]['iters'].tolist()}, unfinished at {rc.CUT[model]}: {n_cut}")
    assert n_cut >= 1                                            # the cut did cut something
    if model == "srbd13" and case == "base":
        assert n_cut < rc.SHAPES[model][1]                       # ... and left finished instances beside them
    same_bytes(two, ref, msg="(cut, continued)")
    same_bytes(three, ref, msg="(cut, continued, continued)")


# ---- 2. the cut itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,wps", [("srbd13", 1), ("srbd13", 2), ("srbd37", 2), ("srbd61", 1)])
def test_the_cut_of_a_resumable_handle_is_the_cut_of_an_ordinary_one(model, wps):
    b = rc.batch(model)
    plain, res = resume_engine(model, "base", wps, resume=False), resume_engine(model, "base", wps)
    same_bytes(cut(res, b, rc.CUT[model]), cut(plain, b, rc.CUT[model]))
    res.enable_resume(False)                                     # and back on the ordinary kernels
    same_bytes(cut(res, b, rc.TOTAL), uncut(model, "base", wps))
    plain.close(); res.close()


# ---- 3. finished instances are left alone; the count ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["srbd13", "srbd37"])
def test_a_continue_launch_leaves_finished_instances_alone(model):
    b = rc.batch(model)
    eng = resume_engine(model, "base", 2)
    assert eng.unfinished() == 0                                 # never solved
    at_cut = cut(eng, b, rc.CUT[model])
    open_ = at_cut[2]["status"] == 1
    assert eng.unfinished() == int(open_.sum()) and 0 < open_.sum()
    lo = rc.SHAPES[model][1] // 4
    assert eng.unfinished(lo, 2 * lo) == int(open_[lo:3 * lo].sum())
    done = continue_to(eng, rc.TOTAL)
    same_bytes(done, at_cut, sel=~open_, msg="(instances with flag 0)")
    same_bytes(done, uncut(model, "base", 2))
    assert (done[2]["status"] != 1).all() and eng.unfinished() == 0
    again = continue_to(eng, rc.TOTAL)                             # nothing left to continue: nothing changes
    same_bytes(again, done)
    eng.close()


# ---- 4. ranges and order -------------------------------------------------------------------------------------------------------------
def test_a_range_continues_its_instances_only():
    model = "srbd13"
    b, ref, B = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model][1]
    eng = resume_engine(model, "base", 2)
    at_cut = cut(eng, b, rc.CUT[model])
    lo, n = 8, 16
    got = continue_to(eng, rc.TOTAL, lo, n)
    inside = np.zeros(B, dtype=bool); inside[lo:lo + n] = True
    assert (at_cut[2]["status"][inside] == 1).any() and (at_cut[2]["status"][~inside] == 1).any()
    same_bytes(got, at_cut, sel=~inside, msg="(outside the range)")
    same_bytes(got, ref, sel=inside, msg="(inside the range)")
    eng.close()


@pytest.mark.parametrize("order", [0, 1, 2])
def test_two_halves_in_either_order_under_every_queue_order(order):
    model = "srbd13"
    b, ref, B = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model][1]
    eng = resume_engine(model, "base", 2, queue_order=order)
    for halves in (((0, B // 2), (B // 2, B // 2)), ((B // 2, B // 2), (0, B // 2))):
        cut(eng, b, rc.CUT[model])
        eng.set_options(max_iters=rc.TOTAL)
        for lo, n in halves:
            eng.continue_solve(None, lo, n)
            assert eng.queue_info()[1:] == (rc.MAX_SLOTS[model], n)          # a queue on few slots
        same_bytes(snap(eng), ref, msg=f"(queue_order {order}, halves {halves})")
    eng.close()


# ---- 5. invalidation and errors -----------------------------------------------------------------------------------------------------
def test_rewritten_instances_cannot_be_continued():
    model = "srbd13"
    b, ref, (N, B) = rc.batch(model), uncut(model, "base", 2), rc.SHAPES[model]
    eng = resume_engine(model, "base", 2)
    at_cut = cut(eng, b, rc.CUT[model])
    open_ = at_cut[2]["status"] == 1
    lo, n = 4, 20
    assert open_[lo:lo + n].any() and open_[lo + n:].any()
    x0 = torch.from_numpy(b["x0"][lo:lo + n].copy()).to("cuda:0")
    torch.cuda.synchronize()
    eng.load_range_device(lo, n, x0=x0)                          # the same values: xs / us / stats keep their bytes
    touched = np.zeros(B, dtype=bool); touched[lo:lo + n] = True
    assert eng.unfinished() == int((open_ & ~touched).sum())
    got = continue_to(eng, rc.TOTAL)
    same_bytes(got, at_cut, sel=touched, msg="(sddp_load_range_device: invalidated)")
    same_bytes(got, ref, sel=~touched, msg="(the others)")
    # sddp_advance rewrites every instance
    eng.set_options(max_iters=rc.CUT[model])
    eng.load(b["x0"], b["xs"], b["us"]); eng.set_params(b["params"]); eng.solve_resident()
    assert eng.unfinished() == int(open_.sum())
    eng.advance(b["params"][:, -1], b["x0"])
    assert eng.unfinished() == 0
    before = snap(eng)
    same_bytes(continue_to(eng, rc.TOTAL), before, msg="(sddp_advance: invalidated)")
    eng.close()


def test_continue_is_refused_where_it_cannot_work():
    model = "srbd13"
    b = rc.batch(model)
    eng = resume_engine(model, "base", resume=False)
    cut(eng, b, rc.CUT[model])
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        eng.continue_solve()
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        eng.unfinished()
    eng.close()
    eng = resume_engine(model, "base")
    eng.load(b["x0"], b["xs"], b["us"])
    with pytest.raises(RuntimeError, match="no solve has run|no resident parameters"):
        eng.continue_solve()
    P = torch.from_numpy(b["params"].copy()).to("cuda:0")
    with pytest.raises(RuntimeError, match="no solve has run"):
        eng.continue_solve(P)
    same_bytes(cut(eng, b, rc.TOTAL), uncut(model, "base", 1))       # the handle stays usable
    eng.close()
    for kw in (dict(consts=dict(b["consts"], friction_barrier_weight=1e-3)), dict(second_order=2)):
        eng = resume_engine(model, "base", resume=False, **kw)
        with pytest.raises(RuntimeError, match="plain builds only"):
            eng.enable_resume()
        cut(eng, b, rc.CUT[model])
        with pytest.raises(RuntimeError, match="sddp_enable_resume"):
            eng.continue_solve()
        eng.close()
    # lip30 has one build and takes second_order = 2 through sddp_set_options: not together with resumable solves, either way round
    lip = resume_engine("lip30", "base", 2)
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
    b, (N, B) = rc.batch(model), rc.SHAPES[model]
    over, _ = draw(b["consts"], B, SRBD13_FIELDS if model == "srbd13" else TRACKING, seed=7)
    plain = resume_engine(model, "base", 2, resume=False)
    plain.set_instance_consts(over)
    ref = cut(plain, b, rc.TOTAL)
    assert (ref[2]["iters"] != uncut(model, "base", 2)[2]["iters"]).any()      # a heterogeneous batch indeed
    eng = resume_engine(model, "base", 2)
    eng.set_instance_consts(over)                                # (clears the flags: before the cut)
    at_cut = cut(eng, b, rc.CUT[model])
    assert (at_cut[2]["status"] == 1).any()
    same_bytes(continue_to(eng, rc.TOTAL), ref)
    plain.close(); eng.close()


# ---- 7. against the oracle -------------------------------------------------------------------------------------------------------------
def test_the_continued_solve_agrees_with_the_c_oracle():
    """tolerances: parity.assert_matches_c_oracle.  Pins that the two halves together still agree with the oracle, not the path."""
    model = "srbd13"
    b = rc.batch(model)
    eng = resume_engine(model, "base", 2)
    cut(eng, b, rc.CUT[model])
    x, u, st = continue_to(eng, rc.TOTAL)
    eng.close()
    parity.assert_matches_c_oracle(x, u, st, *rc.oracle(model, "base"))


# ---- 8. policy behind a continue ---------------------------------------------------------------------------------------------------
def test_the_policy_behind_the_last_slice_is_the_policy_behind_the_uncut_solve():
    model = "srbd13"
    b = rc.batch(model)
    plain, eng = resume_engine(model, "base", 2, resume=False), resume_engine(model, "base", 2)
    recs = []
    for e, cuts in ((plain, ()), (eng, (rc.CUT[model],))):
        e.enable_policy(1)
        cut(e, b, cuts[0] if cuts else rc.TOTAL)
        if cuts:
            continue_to(e, rc.TOTAL)
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
    eng = resume_engine(model, "base", 2, queue_order=3)
    eng.set_instance_classes(labels, 3)
    at_cut = cut(eng, b, rc.CUT[model])
    open_ = at_cut[2]["status"] == 1
    for c in range(3):
        mean, n = eng.class_history(c)
        sel = (labels == c) & ~open_
        assert n == sel.sum() and mean * n == pytest.approx(at_cut[2]["iters"][sel].sum())
    same_bytes(continue_to(eng, rc.TOTAL), ref)
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
    eng = resume_engine(model, "base", 2, resume=False)
    q = FleetQueue(eng, dev(b["params"]), B, 1)
    q.submit(dev(b["x0"]), dev(b["xs"]), dev(b["us"]))
    finished, records = q.solve_sliced(rc.CUT[model], rc.TOTAL)
    torch.cuda.synchronize()
    same_bytes(snap(eng), ref)
    fin, rec, first = finished.cpu().numpy(), records.cpu().numpy(), q.first_records.cpu().numpy()
    assert 0 < fin.sum() < B and q.launches == 2
    want = np.concatenate([ref[1][:, 0], ref[0][:, 1], ref[2]["cost"][:, None], ref[2]["iters"][:, None].astype(float)], axis=1)
    assert rec.tobytes() == want.tobytes()
    assert first[fin].tobytes() == want[fin].tobytes()           # what the first slice handed out was final
    assert not eng.resume_enabled and eng.opts.max_iters == rc.TOTAL      # the engine is left as it was found
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        eng.unfinished()
    eng.close()
