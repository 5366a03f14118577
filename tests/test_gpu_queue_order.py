"""The order a queued launch hands its instances out in (sddp_options.queue_order 1, 2, 3), read back through
DdpEngine.last_queue_order and compared with the rules tests/queue_order_cases.py states in numpy, on every kernel family: the
instantiations of queue_cost_key_kernel (plain, `_x`, barrier, second_order = 2, user build, with a table of per-instance constants,
horizons past one and two trips of its knot loop, a launch over a range, non-finite starts), queue_order_kernel (never solved first,
the clamp at 256, more than 1024 instances) and class_key_kernel (class means, the initial-cost tie-break, unlabelled instances and
classes without history, no class table).  What the table can tell apart is asserted on the CPU by
tests/test_queue_order_cases_cpu.py; the consumption of the order by the slots stays with the bit-identity tests.

Every key case also asserts stats.cost at max_iters = 0 against the oracle's J0 (rtol 1e-12): a wrong key and a wrong cost are told
apart.  No number here comes from the library but what a rule names as its input (class sums, previous iteration counts).

Measured on an MI355X: the 33 tests take 6.5 s (the first one loads the library: 2.6 s; the user build 1.0 s; every other under
0.4 s); stats.cost is within 7.8e-16 of the oracle's J0 on every key case and every order is the reference argsort; no library bug
showed.  Deliberate break on a scratch build: the radix sort flipped to ascending fails all 29 tests of orders 2 and 3 here (the four
order 1 tests do not go through the sort) and, of the earlier suite, only the three tests that assert a direction
(test_cold_queue_order_starts_the_costliest_warm_starts_first, test_class_history_orders_the_queue_and_changes_no_result,
test_auto_classes_change_only_where_the_labels_come_from); the other 231 tests of the queue, failure-exit, launch-sequence,
auto-class and instance-constant modules pass on it."""
import numpy as np
import pytest
import torch

from srbd_horizon_amd import workload  # noqa: F401
from srbd_horizon_amd.engine import DdpEngine
from tests import queue_order_cases as qc, user_terms_defs as defs
from tests.gpu_support import solve

pytestmark = pytest.mark.gpu

KEYS = list(qc.KEY_CASES)


def _key_engine(name, order=2, **over):
    c, s = qc.KEY_CASES[name], qc.start(name)
    opts = dict(qc.BASE, max_iters=0, queue_order=order, max_slots=c.slots, **s["opts"])
    opts.update(over)
    if c.wps:
        opts["waves_per_simd"] = c.wps
    mid = defs.user_case(qc.USER_CASE, c.N)[1] if c.build == "user" else None
    eng = DdpEngine(c.model, c.N, c.B, opts=opts, consts=s["consts"], model_id=mid)
    if s["table"] is not None:
        eng.set_instance_consts(s["table"])
    return eng


def _launch(eng, c, s):
    """the case's one launch -> stats of the whole handle"""
    if c.first == 0 and c.count == c.B:
        return solve(eng, s)[2]
    eng.use_torch_stream(torch.cuda.current_stream())
    eng.load(s["x0"], s["xs"], s["us"])
    eng.solve_range_device(torch.from_numpy(np.array(s["params"])).cuda(), c.first, c.count)
    return eng.fetch()[2].copy()


@pytest.mark.parametrize("name", KEYS)
def test_cold_queue_follows_the_initial_costs(name):
    c, s = qc.KEY_CASES[name], qc.start(name)
    J0 = qc.initial_costs(name)
    keys = qc.order2_reference(J0)
    eng = _key_engine(name)
    assert eng.np_ == s["params"].shape[2]
    st = _launch(eng, c, s)
    queue, order = eng.queue_info(), eng.last_queue_order()
    eng.close()
    assert queue[1:] == (c.slots, c.count)
    r = slice(c.first, c.first + c.count)
    fin = np.isfinite(J0[r])
    rel = np.abs(st["cost"][r][fin] / J0[r][fin] - 1.0).max()
    print(f"{name}: stats.cost against the oracle's J0: {rel:.2e} relative")
    np.testing.assert_allclose(st["cost"][r][fin], J0[r][fin], rtol=1e-12)
    assert not np.isfinite(st["cost"][r][~fin]).any()
    ties = qc.assert_follows(order, keys, c.first, c.count, qc.key_tol(J0))
    if c.kind == "nonfinite":                                  # the two non-finite starts lead, in either order
        assert ties == 1 and set(order[:2].tolist()) == {qc.NAN_AT, qc.INF_AT}
        np.testing.assert_array_equal(order[2:], qc.reference_order(keys, 0, c.B)[2:])
    else:
        assert ties == 0
        np.testing.assert_array_equal(order, qc.reference_order(keys, c.first, c.count))


@pytest.mark.parametrize("name", ["srbd13-N30-w1", "srbd37-N20", "srbd13-nonfinite"])
def test_order_3_without_a_class_table_is_order_2(name):
    """(f): launch_solve_sequence falls back to the initial-cost keys where the handle has no class table"""
    c, s = qc.KEY_CASES[name], qc.start(name)
    J0 = qc.initial_costs(name)
    keys = qc.order2_reference(J0)
    eng = _key_engine(name, order=3)
    assert eng.auto_classes_info() == (False, 0)
    _launch(eng, c, s)
    queue, order = eng.queue_info(), eng.last_queue_order()
    eng.close()
    assert queue[1:] == (c.slots, c.count)
    lead = 2 if c.kind == "nonfinite" else 0
    assert qc.assert_follows(order, keys, 0, c.B, qc.key_tol(J0)) == (1 if lead else 0)
    np.testing.assert_array_equal(order[lead:], qc.reference_order(keys, 0, c.B)[lead:])


def test_non_finite_starts_lead_the_class_history_queue():
    """class_key_kernel keeps a non-finite initial cost as the key: both lead under order 3 with a class table and a history"""
    name = "srbd13-nonfinite"
    c, s = qc.KEY_CASES[name], qc.start(name)
    J0 = qc.initial_costs(name)
    labels, ncls = workload.schedule_classes(c.model, s["params"])
    eng = _key_engine(name, order=3, max_iters=qc.BASE["max_iters"])
    eng.set_instance_classes(labels, ncls)
    st1 = solve(eng, s)[2]                                     # the learning solve
    assert (st1["status"][[qc.NAN_AT, qc.INF_AT]] == 3).all()
    hist = eng.class_stats().astype(np.float64)
    eng.set_options(max_iters=0)
    solve(eng, s)
    queue, order = eng.queue_info(), eng.last_queue_order()
    eng.close()
    assert queue[1:] == (c.slots, c.B)
    keys = qc.order3_keys(J0, labels, hist[:, 0], hist[:, 1])
    assert np.isposinf(keys[[qc.NAN_AT, qc.INF_AT]]).all()
    ties = qc.assert_follows(order, keys, 0, c.B, qc.order3_tol(keys))
    assert set(order[:2].tolist()) == {qc.NAN_AT, qc.INF_AT} and 1 <= ties <= qc.order3_ties(keys, 0, c.B)
    np.testing.assert_array_equal(order[2:], qc.reference_order(keys, 0, c.B)[2:])


# ---- order 1 -------------------------------------------------------------------------------------------------------------------------
def _order1_engine(model, N, B, slots, **over):
    eng = DdpEngine(model, N, B, opts=dict(qc.BASE, queue_order=1, max_slots=slots, **over))
    eng.use_torch_stream(torch.cuda.current_stream())
    return eng


def _solve_range(eng, P, first, count, max_iters):
    eng.set_options(max_iters=max_iters)
    eng.solve_range_device(P, first, count)
    return eng.fetch()[2]["iters"][first:first + count].copy()


def test_second_launch_follows_the_first_launchs_iterations():
    """(a): on the first launch every instance is "never solved" (any permutation); the second follows order1_keys, exactly"""
    N, B, slots = 30, 96, 8
    batch = workload.make_batch("srbd13", N, np.arange(B) + 4000)
    eng = _order1_engine("srbd13", N, B, slots)
    st1 = solve(eng, batch)[2]
    assert eng.queue_info()[1:] == (slots, B)
    assert qc.assert_follows(eng.last_queue_order(), qc.order1_keys(np.full(B, -1)), 0, B, 0.0) == B - 1
    solve(eng, batch)
    assert eng.queue_info()[1:] == (slots, B)
    order = eng.last_queue_order()
    eng.close()
    keys = qc.order1_keys(st1["iters"])
    assert len(np.unique(keys)) >= 8 and keys.max() < 256
    assert qc.assert_follows(order, keys, 0, B, 0.0) == qc.order1_ties(keys)


def test_never_solved_instances_come_first():
    """(b): the range [0, 48) solved first, then the whole batch"""
    N, B, slots = 30, 96, 8
    batch = workload.make_batch("srbd13", N, np.arange(B) + 4000)
    eng = _order1_engine("srbd13", N, B, slots)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    P = torch.from_numpy(batch["params"]).cuda()
    it = _solve_range(eng, P, 0, 48, qc.BASE["max_iters"])
    assert eng.queue_info()[1:] == (slots, 48)
    eng.solve_range_device(P, 0, B)
    eng.synchronize()
    assert eng.queue_info()[1:] == (slots, B)
    order = eng.last_queue_order()
    eng.close()
    keys = qc.order1_keys(np.concatenate([it, np.full(48, -1)]))
    assert qc.assert_follows(order, keys, 0, B, 0.0) == qc.order1_ties(keys)
    assert sorted(order[:48].tolist()) == list(range(48, 96))


def test_the_clamp_at_256_iterations():
    """(c): four ranges of one lip30 handle solved to 300, 257, 256 and 200 iterations -- the caps, as on the C oracle --, then the
    whole batch queued: the first three tie at 256, in any order, and precede the fourth"""
    s = qc.c_start()
    eng = DdpEngine(qc.C_MODEL, qc.C_N, qc.B, opts=dict(qc.c_options(), queue_order=1, max_slots=qc.SLOTS), consts=s["consts"])
    eng.use_torch_stream(torch.cuda.current_stream())
    eng.load(s["x0"], s["xs"], s["us"])
    P = torch.from_numpy(np.array(s["params"])).cuda()
    it = []
    for i, cap in enumerate(qc.C_CAPS):
        it.append(_solve_range(eng, P, i * qc.C_RANGE, qc.C_RANGE, cap))
        assert eng.queue_info()[1:] == (qc.SLOTS, qc.C_RANGE)
        np.testing.assert_array_equal(it[-1], qc.c_oracle_iters(cap, "off", i * qc.C_RANGE, qc.C_RANGE))
        assert (it[-1] == cap).all()
    eng.set_options(max_iters=0)
    eng.solve_range_device(P, 0, qc.B)
    eng.synchronize()
    assert eng.queue_info()[1:] == (qc.SLOTS, qc.B)
    order = eng.last_queue_order()
    eng.close()
    keys = qc.order1_keys(np.concatenate(it))
    assert keys.tolist() == [256] * (3 * qc.C_RANGE) + [200] * qc.C_RANGE
    assert qc.assert_follows(order, keys, 0, qc.B, 0.0) == qc.order1_ties(keys) == qc.B - 2
    assert sorted(order[:3 * qc.C_RANGE].tolist()) == list(range(3 * qc.C_RANGE))


def test_more_than_1024_instances_take_the_second_trip_of_the_counting_sort():
    """the launch shape of (c) with count = 1500 > 1024 threads: three ranges solved at max_iters 100, 2, 1, the fourth never"""
    d, s = qc.STRIDE, qc.stride_start()
    B, n = d["B"], d["B"] // 4
    eng = _order1_engine(d["model"], d["N"], B, d["slots"])
    eng.load(s["x0"], s["xs"], s["us"])
    P = torch.from_numpy(np.array(s["params"])).cuda()
    it = [_solve_range(eng, P, i * n, n, cap) for i, cap in enumerate(d["caps"])]
    eng.set_options(max_iters=0)
    eng.solve_range_device(P, 0, B)
    eng.synchronize()
    assert eng.queue_info()[1:] == (d["slots"], B)
    order = eng.last_queue_order()
    eng.close()
    keys = qc.order1_keys(np.concatenate(it + [np.full(n, -1)]))
    print(f"previous iterations: {np.unique(np.concatenate(it), return_counts=True)}")
    assert len(np.unique(keys)) >= 4
    assert qc.assert_follows(order, keys, 0, B, 0.0) == qc.order1_ties(keys)
    assert sorted(order[:n].tolist()) == list(range(3 * n, B))


# ---- order 3 -------------------------------------------------------------------------------------------------------------------------
def _order3_engine(model):
    N, B, slots, wps, _ = qc.ORDER3[model]
    return DdpEngine(model, N, B, opts=dict(qc.BASE, queue_order=3, max_slots=slots, waves_per_simd=wps), consts=qc.order3_start(model)["consts"])


def _learn_then_look(eng, s, labels_learning, labels_final):
    """one learning solve under BASE, then the launch that is looked at (max_iters = 0) -> (class history the launch saw, its order)"""
    B = len(labels_final)
    eng.set_instance_classes(labels_learning, s["n_classes"])
    solve(eng, s)
    eng.set_instance_classes(labels_final, s["n_classes"])
    hist = eng.class_stats().astype(np.float64)
    eng.set_options(max_iters=0)
    st = solve(eng, s)[2]
    assert eng.queue_info()[2] == B
    np.testing.assert_allclose(st["cost"], s["J0"], rtol=1e-12)
    return hist, eng.last_queue_order()


@pytest.mark.parametrize("model", list(qc.ORDER3))
def test_class_history_queue_follows_the_class_means_and_the_initial_cost_inside_a_class(model):
    """(d)"""
    s = qc.order3_start(model)
    B = qc.ORDER3[model][1]
    eng = _order3_engine(model)
    hist, order = _learn_then_look(eng, s, s["labels"], s["labels"])
    eng.close()
    assert hist[:, 1].sum() == B and (hist[np.unique(s["labels"]), 1] > 0).all()
    keys = qc.order3_keys(s["J0"], s["labels"], hist[:, 0], hist[:, 1])
    declared = qc.order3_ties(keys, 0, B)
    print(f"{model}: class means {np.unique(np.floor(keys)).tolist()}; declared ties {declared}")
    assert qc.assert_follows(order, keys, 0, B, qc.order3_tol(keys)) <= declared
    if declared == 0:
        np.testing.assert_array_equal(order, qc.reference_order(keys, 0, B))
    for c in np.unique(s["labels"]):                           # inside every class: descending initial cost
        mine = order[s["labels"][order] == c]
        assert (np.diff(s["J0"][mine]) < 0).all(), c


@pytest.mark.parametrize("model", list(qc.ORDER3))
def test_unlabelled_instances_and_classes_without_history_lead(model):
    """(e)"""
    s = qc.order3_start(model)
    B = qc.ORDER3[model][1]
    learning, final, unseen = qc.order3_labels_e(model)
    eng = _order3_engine(model)
    hist, order = _learn_then_look(eng, s, learning, final)
    eng.close()
    assert hist[unseen, 1] == 0 and hist[:, 1].sum() == (learning >= 0).sum()
    keys = qc.order3_keys(s["J0"], final, hist[:, 0], hist[:, 1])
    lead = (final < 0) | (final == unseen)
    n = int(lead.sum())
    assert (keys[lead] > 9e5).all() and (keys[~lead] < 200).all()
    assert qc.assert_follows(order, keys, 0, B, qc.order3_tol(keys)) <= qc.order3_ties(keys, 0, B)
    assert sorted(order[:n].tolist()) == np.flatnonzero(lead).tolist()
    rest = -np.sort(-keys[~lead])                              # behind the leaders: the reference order, where no two keys are within an ulp
    if (np.abs(np.diff(rest)) > np.spacing(rest.max())).all():
        np.testing.assert_array_equal(order[n:], qc.reference_order(keys, 0, B)[n:])
    far = np.abs(np.diff(s["J0"][order[:n]])) > 2 * 116.0 * 1.2                        # among them: descending J0 wherever the key resolves it
    assert (np.diff(s["J0"][order[:n]])[far] < 0).all()
