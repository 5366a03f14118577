"""Masked launches on the GPU (include/sddp.h sddp_*_masked_device): a selected instance gets the range launch's bytes, an
unselected one keeps every byte it had, on a one-wave build (srbd13) and a four-wave build (lip30), with a real queue (max_slots =
8: more selected instances than slots) and with the default slots (fewer selected than slots).  Every comparison is bitwise.
B = 48 at the horizons of tests/resume_cases.py; max_iters = 6 except where a test needs the uncut solve."""
import functools

import numpy as np
import pytest
import torch

from srbd_horizon_amd import _lib, workload
from srbd_horizon_amd.engine import DdpEngine
from tests import gpu_support as gs, masked_cases as mc, oracle_refs as refs

pytestmark = pytest.mark.gpu

B, ITERS, TOTAL = mc.B, 6, 100
WPS = {"srbd13": 1, "lip30": 2}
CUT = {"srbd13": 2, "lip30": 1}                          # max_iters that leaves unfinished instances
MODELS = sorted(mc.SHAPES)
BUILDS = [(m, s) for m in MODELS for s in (8, 0)]        # max_slots: 8 = a queue on few slots; 0 = every resident workgroup


def batch(model, other=False):
    """the batch the masked launches run on (seeds 0 .. 47); other: the one whose solve fills the handle first (seeds 100 .. 147)"""
    return refs.batch(model, mc.SHAPES[model], range(100, 100 + B) if other else range(B))


def engine(model, slots=8, resume=False, log=0, **over):
    opts = refs.options(dict(max_iters=ITERS, max_slots=slots, waves_per_simd=WPS[model]), **over)
    eng = DdpEngine(model, mc.SHAPES[model], B, opts=opts, consts=batch(model)["consts"])
    eng.use_torch_stream(torch.cuda.current_stream())
    if resume:
        eng.enable_resume()
    if log:
        eng.enable_iteration_log(log)
    return eng


def imask(m):
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)).to("cuda")


@functools.lru_cache(maxsize=None)
def twin(model, max_iters=ITERS):
    """sddp_solve_range_device over everything on a handle of its own (default queue order and slots): computed once, read-only"""
    eng = engine(model, 0, max_iters=max_iters)
    a = batch(model)
    eng.load(a["x0"], a["xs"], a["us"])
    eng.solve_range_device(gs.dev(a["params"]), 0, B)
    out = gs.snap(eng)
    eng.close()
    return gs.frozen(out)


@functools.lru_cache(maxsize=None)
def initial_costs(model):
    """the total cost of every warm start, the key of queue order 2: what a solve at max_iters = 0 reports"""
    return gs.frozen(twin(model, 0)[2]["cost"].copy())


def filled(eng, model, a=None):
    """the handle after a solve of the OTHER batch (every instance holds a plan, stats, a previous iteration count), loaded with the
    start of batch `a`; -> (the device parameters of `a`, the handle's bytes before the launch)"""
    gs.solve(eng, batch(model, other=True))
    a = batch(model) if a is None else a
    eng.load(a["x0"], a["xs"], a["us"])
    return gs.dev(a["params"]), gs.snap(eng)


def words(eng):
    """(SDDP_BUF_ORDER, SDDP_BUF_SELECTED) of the last launch on the host"""
    return eng._host_copy(_lib.BUF_ORDER, "<i4"), eng._host_copy(_lib.DEVICE_BUF_SELECTED, "<i4")


def flags(eng):
    return np.array([eng.unfinished(b, 1) for b in range(B)])


# ---- 1 (and the first half of 5): equality under every queue order, the pre-pass against its numpy statement, the class history ----------
@pytest.mark.parametrize("queue_order", [0, 1, 2, 3])
@pytest.mark.parametrize("model,slots", BUILDS)
def test_selected_instances_get_the_range_launch_and_the_others_keep_their_bytes(model, slots, queue_order):
    ref, m = twin(model), mc.mask_half(B)
    sel = m != 0
    eng = engine(model, slots, queue_order=queue_order)
    labels = (np.arange(B) * 7 % 5 - 1).astype(np.int32)                     # -1 (unlabelled) and the classes 0 .. 3
    if queue_order == 3:
        eng.set_instance_classes(labels, 4)
    P, before = filled(eng, model)
    hist = before[2]["iters"].copy()                                           # the previous solve's iteration counts
    stat0 = eng.class_stats() if queue_order == 3 else None
    eng.solve_masked_device(P, imask(m))
    after = gs.snap(eng)
    gs.same_bytes(after, ref, sel, "selected")
    gs.same_bytes(after, before, ~sel, "unselected")
    assert eng.last_selected() == sel.sum()
    assert eng.queue_info()[2] == B and eng.queue_info()[1] == (min(8, B) if slots else min(B, eng.queue_info()[0]))
    order, selw = words(eng)
    key = mc.keys(queue_order, B, hist, initial_costs(model), labels, stat0)
    print(f"{model} slots {slots} order {queue_order}: n_selected, queue start {selw.tolist()}; hand-out {order[selw[1]:].tolist()}")
    mc.check_prepass(order, selw, m, 0, key)
    with pytest.raises(RuntimeError, match="per queue slot"):
        eng.device_buffer(_lib.BUF_GAINS)
    if queue_order == 3:      # the class history grew by exactly the iterations and the count of the selected, labelled instances
        grown = eng.class_stats().astype(np.int64) - stat0.astype(np.int64)
        want = np.array([[ref[2]["iters"][sel & (labels == c)].sum(), np.count_nonzero(sel & (labels == c))] for c in range(4)])
        np.testing.assert_array_equal(grown, want)
    # the previous iteration counts (the key of queue_order = 1) of the unselected instances are still the first solve's: a second
    # masked launch under order 1, with another mask, hands out by them
    m2 = mc.mask_half(B, seed=9)
    eng.set_options(queue_order=1)
    eng.solve_masked_device(P, imask(m2))
    order, selw = words(eng)
    assert (m2 != 0)[~sel].sum() > 1                                             # kept keys are handed out ...
    assert model != "srbd13" or len(set(hist[~sel & (m2 != 0)].tolist())) > 1   # ... and differ (lip30: two iterations everywhere)
    mc.check_prepass(order, selw, m2, 0, mc.keys(1, B, np.where(sel, ref[2]["iters"], hist)))
    # the next unmasked launch is an ordinary one again
    eng.solve_range_device(P, 0, B)
    assert eng.queue_info()[2] == (B if slots else 0)
    eng.close()


# ---- 2: edge masks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,slots", BUILDS)
def test_edge_masks(model, slots):
    ref, a = twin(model), batch(model)
    eng = engine(model, slots)
    P, _ = filled(eng, model)
    cases = [(name, 0, m) for name, m in mc.edge_masks(B).items()]
    cases += [("count 1", 5, np.ones(1, np.int32)), ("count 1, unselected", 6, np.zeros(1, np.int32)),
              ("first > 0", 7, mc.mask_half(20, seed=2)), ("first > 0, its edges", 30, np.eye(1, 18, 17, dtype=np.int32)[0] + np.eye(1, 18, 0, dtype=np.int32)[0])]
    for name, first, m in cases:
        eng.load(a["x0"], a["xs"], a["us"])
        before = gs.snap(eng)
        eng.solve_masked_device(P, imask(m), first, len(m))
        after = gs.snap(eng)
        sel = np.zeros(B, bool)
        sel[first:first + len(m)] = m != 0
        gs.same_bytes(after, ref, sel, f"selected ({name})")
        gs.same_bytes(after, before, ~sel, f"unselected ({name})")
        assert eng.last_selected() == sel.sum(), name
        order, selw = words(eng)
        mc.check_prepass(order, selw, m, first, mc.keys(1, len(m), before[2]["iters"][first:first + len(m)]))      # (the default order: 1)
        assert eng.queue_info()[2] == len(m)
    eng.close()


# ---- 3: the partition under bad keys ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,slots", BUILDS)
def test_a_selected_instance_with_a_nan_start_is_solved_and_no_unselected_one_is(model, slots):
    ref, m = twin(model), mc.mask_half(B)
    sel = m != 0
    nan_b = int(np.flatnonzero(sel)[3])
    a = dict(batch(model))
    a["x0"] = np.array(a["x0"])
    a["x0"][nan_b, 0] = np.nan
    eng = engine(model, slots, queue_order=2)
    P, before = filled(eng, model, a)
    eng.solve_masked_device(P, imask(m))
    after = gs.snap(eng)
    assert after[2]["status"][nan_b] == 3
    others = sel.copy()
    others[nan_b] = False
    gs.same_bytes(after, ref, others, "the other selected instances")
    gs.same_bytes(after, before, ~sel, "unselected")
    cost = np.array(initial_costs(model))
    cost[nan_b] = np.nan
    order, selw = words(eng)
    mc.check_prepass(order, selw, m, 0, mc.keys(2, B, cost=cost))
    assert order[selw[1]] == nan_b                                             # first among the selected, behind every unselected instance
    eng.close()


# ---- 4: resume ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,slots", BUILDS)
def test_a_masked_launch_keeps_the_cut_solves_of_the_unselected_instances(model, slots):
    full, m, a = twin(model, TOTAL), mc.mask_half(B), batch(model)
    sel = m != 0
    eng = engine(model, slots, resume=True, log=8)
    before = gs.cut(eng, a, CUT[model])
    f0, log0 = flags(eng), gs.log_of(eng)
    assert f0[~sel].sum() > 0 and f0[sel].sum() > 0                            # unfinished instances on both sides of the mask
    eng.set_options(max_iters=TOTAL)
    for b in np.flatnonzero(sel):                                               # the selected instances start afresh (which clears THEIR flags)
        eng.load_range_device(int(b), 1, gs.dev(a["x0"][b:b + 1]), gs.dev(a["xs"][b:b + 1]), gs.dev(a["us"][b:b + 1]))
    eng.solve_masked_device(None, imask(m))
    after = gs.snap(eng)
    gs.same_bytes(after, full, sel, "selected: the uncut solve")
    gs.same_bytes(after, before, ~sel, "unselected: the cut iterate")
    f1, log1 = flags(eng), gs.log_of(eng)
    np.testing.assert_array_equal(f1[~sel], f0[~sel])
    assert log1[0][~sel].tobytes() == log0[0][~sel].tobytes() and log1[1][~sel].tobytes() == log0[1][~sel].tobytes()
    # the carry rows survived: the range continue finishes the unselected instances to the bytes of the uncut solve
    gs.same_bytes(gs.continue_to(eng, TOTAL), full, slice(None), "continued")
    # sddp_continue_masked_device: the selected instances with flag 1 alone
    cutb = gs.cut(eng, a, CUT[model])
    f2 = flags(eng)
    eng.set_options(max_iters=TOTAL)
    eng.continue_masked(imask(m))
    after = gs.snap(eng)
    gs.same_bytes(after, full, sel & (f2 == 1), "selected and unfinished")
    gs.same_bytes(after, cutb, ~(sel & (f2 == 1)), "everything else")
    np.testing.assert_array_equal(flags(eng), np.where(sel, 0, f2))
    assert eng.last_selected() == sel.sum()
    eng.close()


# ---- 5, second half: auto classes relabel the selected instances alone ------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_auto_classes_relabel_selected_instances_only(model):
    m = mc.mask_half(B)
    sel = m != 0
    eng = engine(model, 8, queue_order=3)
    eng.enable_auto_classes()
    P, _ = filled(eng, model)
    old = eng.instance_classes().copy()
    new = workload.schedule_classes(model, np.asarray(batch(model)["params"]))[0]
    np.testing.assert_array_equal(old, workload.schedule_classes(model, np.asarray(batch(model, other=True)["params"]))[0])
    assert (old != new)[~sel].any() and (old != new)[sel].any()                # the test can tell a relabelled instance from a kept one
    stat0 = eng.class_stats().astype(np.int64)
    eng.solve_masked_device(P, imask(m))
    np.testing.assert_array_equal(eng.instance_classes(), np.where(sel, new, old))
    grown = eng.class_stats().astype(np.int64) - stat0
    iters = gs.snap(eng)[2]["iters"]
    want = np.zeros_like(grown)
    for b in np.flatnonzero(sel):
        want[new[b]] += (iters[b], 1)
    np.testing.assert_array_equal(grown, want)
    eng.close()


# ---- 6: policy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,slots", BUILDS)
def test_masked_policy_records(model, slots):
    m, a = mc.mask_half(B), batch(model)
    sel = m != 0

    def handle():
        eng = engine(model, slots)
        eng.enable_policy(3)
        eng.enable_value(2)
        return eng

    ref = handle()
    ref.load(a["x0"], a["xs"], a["us"])
    ref.solve_range_device(gs.dev(a["params"]), 0, B)
    ref.policy_range_device()
    want = ref.fetch_policy().copy(), ref.fetch_value().copy()
    ref.close()
    eng = handle()
    gs.solve(eng, batch(model, other=True))
    eng.policy_range_device()                                                  # the records of the other batch's plans: the earlier bytes
    early = eng.fetch_policy().copy(), eng.fetch_value().copy()
    eng.load(a["x0"], a["xs"], a["us"])
    P = gs.dev(a["params"])
    eng.solve_range_device(P, 0, B)
    plan = gs.snap(eng)
    eng.policy_masked_device(imask(m))
    got = eng.fetch_policy(), eng.fetch_value()
    for g, w, e in zip(got, want, early):
        assert g[sel].tobytes() == w[sel].tobytes() and g[~sel].tobytes() == e[~sel].tobytes()
        assert w[sel].tobytes() != e[sel].tobytes()
    gs.same_bytes(gs.snap(eng), plan, slice(None), "no solve result moves")
    eng.policy_masked_device(imask(mc.mask_half(20, seed=2)), 7, 20)           # a sub-range: the rest of the selected records are the range launch's
    eng.policy_masked_device(imask(np.ones(B, np.int32)))
    assert eng.fetch_policy().tobytes() == want[0].tobytes() and eng.fetch_value().tobytes() == want[1].tobytes()
    eng.close()


# ---- 7: advance -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_masked_advance_is_sddp_advance_for_the_selected_instances(model):
    a, first, count = batch(model), 4, 40
    m = mc.mask_half(count, seed=5)
    sel = np.zeros(B, bool)
    sel[first:first + count] = m != 0
    r = np.random.default_rng(1)
    p_last, x0 = r.standard_normal((B, a["params"].shape[2])), r.standard_normal((B, a["x0"].shape[1]))

    def state(eng):
        eng.synchronize()
        P = eng.device_view(_lib.BUF_PARAMS, a["params"].shape).cpu().numpy().copy()
        X0 = eng.device_view(_lib.BUF_X0, a["x0"].shape).cpu().numpy().copy()
        x, u, _ = gs.snap(eng)
        return P, X0, x, u

    tw, eng = engine(model, 8), engine(model, 8, resume=True)
    for e in (tw, eng):
        e.set_params(a["params"])
        gs.cut(e, a, CUT[model])
    f0 = flags(eng)
    assert f0[sel].sum() > 0 and f0[~sel].sum() > 0
    before = state(eng)
    tw.advance(p_last, x0)
    eng.advance_masked_device(imask(m), gs.dev(p_last[first:first + count]), gs.dev(x0[first:first + count]), first, count)
    for got, want, was in zip(state(eng), state(tw), before):
        assert got[sel].tobytes() == want[sel].tobytes() and got[~sel].tobytes() == was[~sel].tobytes()
        assert want[sel].tobytes() != was[sel].tobytes()
    np.testing.assert_array_equal(flags(eng), np.where(sel, 0, f0))
    tw.close()
    eng.close()


# ---- 8: a time budget that never runs out -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,slots", BUILDS)
def test_a_budget_that_never_runs_out_changes_nothing(model, slots):
    m, ends = mc.mask_half(B), []
    for budget in (0.0, 60e6):
        eng = engine(model, slots, resume=True, queue_order=2)
        eng.set_time_budget(budget)
        P, _ = filled(eng, model)
        eng.solve_masked_device(P, imask(m))
        gs.same_bytes(gs.snap(eng), twin(model), m != 0, f"budget {budget}")
        ends.append(tuple(x.tobytes() for x in gs.snap(eng)) + (flags(eng).tobytes(), words(eng)[0].tobytes()))
        if budget:
            start, deadline = eng.deadline_clock()
            assert deadline - start == int(100 * budget) and int(eng.slot_times()[:, 0].min()) >= start      # the stamp led the sequence
        eng.close()
    assert ends[0] == ends[1]


# ---- 9: refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    model = "srbd13"
    a, m = batch(model), imask(np.ones(B, np.int32))
    eng = engine(model)
    P = gs.dev(a["params"])
    null, vp = None, lambda t: eng._dev(t, t.shape)      # noqa: E731
    mp = DdpEngine._mask(m, B)
    pl, x0 = gs.dev(np.zeros((B, eng.np_))), gs.dev(np.zeros((B, eng.nx)))
    lib, h = eng.lib, eng.h

    def refused(rc, match):
        assert rc == -1                                                         # SDDP_ERR_ARG
        with pytest.raises(RuntimeError, match=match):
            eng._chk(rc)

    eng.load(a["x0"], a["xs"], a["us"])
    refused(lib.sddp_policy_masked_device(h, 0, B, mp), "sddp_enable_policy")
    refused(lib.sddp_continue_masked_device(h, vp(P), 0, B, mp), "sddp_enable_resume")
    refused(lib.sddp_advance_masked_device(h, 0, B, mp, vp(pl), vp(x0)), "resident parameters")
    eng.enable_resume()
    refused(lib.sddp_continue_masked_device(h, vp(P), 0, B, mp), "no solve has run")
    eng.enable_policy(2)
    refused(lib.sddp_policy_masked_device(h, 0, B, mp), "no solve has run")
    eng.set_params(a["params"])
    eng.solve_masked_device(P, m)
    refused(lib.sddp_solve_masked_device(h, vp(P), 0, B, null), "mask is NULL")
    refused(lib.sddp_continue_masked_device(h, vp(P), 0, B, null), "mask is NULL")
    refused(lib.sddp_policy_masked_device(h, 0, B, null), "mask is NULL")
    refused(lib.sddp_advance_masked_device(h, 0, B, null, vp(pl), vp(x0)), "mask is NULL")
    refused(lib.sddp_advance_masked_device(h, 0, B, mp, null, vp(x0)), "both required")
    refused(lib.sddp_advance_masked_device(h, 0, B, mp, vp(pl), null), "both required")
    for first, count in ((-1, 4), (B - 3, 4), (0, 0), (0, B + 1)):
        refused(lib.sddp_solve_masked_device(h, vp(P), first, count, mp), "range outside")
        refused(lib.sddp_continue_masked_device(h, vp(P), first, count, mp), "range outside")
        refused(lib.sddp_policy_masked_device(h, first, count, mp), "range outside")
        refused(lib.sddp_advance_masked_device(h, first, count, mp, vp(pl), vp(x0)), "range outside")
    with pytest.raises(ValueError, match="mask of shape"):
        eng.solve_masked_device(P, m, 0, B - 1)
    assert eng.last_selected() == B                                            # and the handle still works
    gs.same_bytes(gs.snap(eng), twin(model), slice(None), "all ones: the range launch")
    eng.close()
