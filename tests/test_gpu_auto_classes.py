"""Queue order 3 without caller labels (include/sddp.h sddp_enable_auto_classes): the handle labels the instances of every fresh
solve launch itself, by one small kernel in front of the launch sequence, from the parameter tensor the launch runs on.

The labels are integers and everything compared here is `==`: the device labels against workload.schedule_classes (whose own
agreement with the labels written down with the hand-built cases tests/test_auto_classes_cpu.py asserts), results, iteration
counts, class statistics and queue orders of a handle with auto classes against those of a handle the caller labelled.  The
labelling tests solve at max_iters = 0: the starting point is evaluated, nothing iterates, the label kernel runs all the same."""
import numpy as np
import pytest
import torch

from srbd_horizon_amd import workload
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.fleet import FleetQueue
from tests import auto_class_cases as acc
from tests.gpu_support import solve as _solve

pytestmark = pytest.mark.gpu

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)      # dsrbd_example.py:55-58
QUEUE3 = dict(OPTS, max_slots=16, waves_per_simd=2, queue_order=3)         # the shape of test_gpu_queue's class-history test


def _load(eng, b):
    eng.load(b["x0"], b["xs"], b["us"])


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.array(a), dtype=dtype, device="cuda")


def _history(labels, iters, n_classes):
    """[n_classes, 2] uint64: sum of iterations, solves of every class"""
    out = np.zeros((n_classes, 2), dtype=np.uint64)
    np.add.at(out[:, 0], labels, iters.astype(np.uint64))
    np.add.at(out[:, 1], labels, np.uint64(1))
    return out


# ---- 1. the labels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,B,extra", [("srbd13", 30, 37, 0), ("srbd13", 70, 37, 0), ("srbd37", 8, 8, 0), ("lip30", 8, 8, 0),
                                             ("srbd61", 8, 8, 0), ("srbd13", 30, 37, 8)])
def test_device_labels_equal_the_numpy_labels(model, N, B, extra):
    """N = 70: two chunks of 64 nodes; B = 37 and the ranges: count % 4 != 0 (four instances per workgroup); extra = 8: an `_x`
    handle, whose parameter rows are 8 columns wider."""
    c = acc.build(model, N, B, extra)
    want, n_classes = workload.schedule_classes(model, c["params"])
    a = np.zeros(8); a[0] = 1.0
    consts = dict(c["consts"], extra_rows=[dict(a=a, w=1.0, kind="state")]) if extra else c["consts"]
    eng = DdpEngine(model, N, B, opts=dict(OPTS, max_iters=0), consts=consts)
    eng.use_torch_stream(torch.cuda.current_stream())
    assert eng.np_ == c["params"].shape[2]
    assert eng.auto_classes_info() == (False, 0)
    eng.enable_auto_classes()
    assert eng.auto_classes_info() == (True, n_classes) and n_classes == 36 * (N + 2)
    np.testing.assert_array_equal(eng.instance_classes(), np.full(B, -1))
    _load(eng, c)
    first, count = (5, 6) if B >= 11 else (3, 3)
    eng.solve_range_device(_dev(c["params"]), first, count)                # a range: the other labels stay what they were
    part = np.full(B, -1, dtype=np.int32)
    part[first:first + count] = want[first:first + count]
    np.testing.assert_array_equal(eng.instance_classes(), part)
    np.testing.assert_array_equal(eng.instance_classes(first, count), want[first:first + count])
    eng.solve(c["params"])                                                 # the whole batch, through the host entry point
    got = eng.instance_classes()
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    ptr, nbytes = eng.device_buffer(12)
    assert ptr and nbytes == 4 * B
    eng.close()


# ---- 2. nothing else moves ------------------------------------------------------------------------------------------------------
def test_auto_classes_change_only_where_the_labels_come_from():
    N, B = 30, 192
    batch = workload.make_batch("srbd13", N, np.arange(B) + 100)
    labels, n_classes = workload.schedule_classes("srbd13", batch["params"])
    present = np.unique(labels)
    assert len(present) >= 6
    ref = DdpEngine("srbd13", N, B, opts=OPTS)                             # one workgroup per instance, no queue
    x0, u0, s0 = _solve(ref, batch)
    host = DdpEngine("srbd13", N, B, opts=QUEUE3)
    host.set_instance_classes(labels, n_classes)
    auto = DdpEngine("srbd13", N, B, opts=QUEUE3)
    auto.enable_auto_classes()
    for launch in range(2):
        xh, uh, sh = _solve(host, batch)
        oh = host.last_queue_order()
        xa, ua, sa = _solve(auto, batch)
        oa = auto.last_queue_order()
        assert auto.queue_info()[1:] == host.queue_info()[1:] == (16, B)
        np.testing.assert_array_equal(xa, xh); np.testing.assert_array_equal(ua, uh)
        np.testing.assert_array_equal(xa, x0); np.testing.assert_array_equal(ua, u0)
        np.testing.assert_array_equal(sa["iters"], sh["iters"])
        np.testing.assert_array_equal(sa["iters"], s0["iters"])
        np.testing.assert_array_equal(oa, oh, err_msg=f"queue order of launch {launch}")
        for c in present:
            assert auto.class_history(int(c)) == host.class_history(int(c))
            assert auto.class_history(int(c))[1] == (launch + 1) * int((labels == c).sum())
    np.testing.assert_array_equal(auto.instance_classes(), labels)
    assert sorted(oa.tolist()) == list(range(B))
    means = {int(c): s0["iters"][labels == c].mean() for c in present}
    km = np.array([means[int(labels[i])] for i in oa])
    assert np.all(np.diff(km) <= 1e-9)                                     # descending class means along the second launch's order


# ---- 3. every launch labels the tensor it runs on -----------------------------------------------------------------------------
def test_a_launch_after_advance_labels_the_shifted_parameters():
    N, B = 30, 37
    batch = workload.make_batch("srbd13", N, np.arange(B) + 100)
    eng = DdpEngine("srbd13", N, B, opts=dict(OPTS, max_iters=0))
    eng.enable_auto_classes()
    _load(eng, batch)
    P = np.array(batch["params"])
    eng.set_params(P)
    eng.solve_resident()
    before = eng.instance_classes()
    np.testing.assert_array_equal(before, workload.schedule_classes("srbd13", P)[0])
    for tick in range(2):
        p_last = P[:, N].copy()
        p_last[:, 17:19] = 1.0 - p_last[:, 17:19]                          # a contact switch enters at the end of the horizon
        p_last[:, 0] = -p_last[:, 0] if tick else 0.0                      # ... and another command
        P = np.concatenate([P[:, 1:], p_last[:, None]], axis=1)
        eng.advance(p_last, batch["x0"])
        np.testing.assert_array_equal(eng.instance_classes(), before)      # the shift alone relabels nothing: the launch does
        eng.solve_resident()
        after = eng.instance_classes()
        np.testing.assert_array_equal(after, workload.schedule_classes("srbd13", P)[0])
        assert (after != before).any()
        before = after
    eng.close()


# ---- 4. continue launches -------------------------------------------------------------------------------------------------------
def test_a_continue_launch_keeps_the_labels_and_counts_every_instance_once():
    N, B = 30, 48
    batch = workload.make_batch("srbd13", N, np.arange(B) + 100)
    labels, n_classes = workload.schedule_classes("srbd13", batch["params"])
    eng = DdpEngine("srbd13", N, B, opts=dict(OPTS, max_iters=3, max_slots=4))
    eng.use_torch_stream(torch.cuda.current_stream())
    eng.enable_resume()
    eng.enable_auto_classes()
    _load(eng, batch)
    eng.solve_range_device(_dev(batch["params"]), 0, B)
    _, _, cut = eng.fetch()
    cut = cut.copy()
    resumable = cut["status"] == 1
    assert 0 < int(resumable.sum())
    np.testing.assert_array_equal(eng.instance_classes(), labels)
    np.testing.assert_array_equal(eng.class_stats(), _history(labels[~resumable], cut["iters"][~resumable], n_classes))
    # the continue launch gets a tensor that would be labelled differently (the commands at node N reversed): it must not relabel
    P2 = np.array(batch["params"])
    P2[:, N, 0:2] = -P2[:, N, 0:2]
    assert (workload.schedule_classes("srbd13", P2)[0] != labels).any()
    eng.set_options(max_iters=100)
    eng.continue_solve(_dev(P2), 0, B)
    _, _, end = eng.fetch()
    np.testing.assert_array_equal(eng.instance_classes(), labels)
    done = end["status"] != 1
    assert int(done.sum()) >= B - 2                                        # (an instance may crawl to the cap: it is not counted)
    stats = eng.class_stats()
    np.testing.assert_array_equal(stats, _history(labels[done], end["iters"][done], n_classes))
    if done.all():
        np.testing.assert_array_equal(stats[:, 1], np.bincount(labels, minlength=n_classes).astype(np.uint64))
    eng.close()


# ---- 5. the history leaves a handle and enters another ----------------------------------------------------------------------------
def test_class_stats_seed_another_handle():
    N, B = 30, 192
    batch = workload.make_batch("srbd13", N, np.arange(B) + 100)
    a = DdpEngine("srbd13", N, B, opts=QUEUE3)
    a.enable_auto_classes()
    n_classes = a.auto_classes_info()[1]
    assert a.class_stats().shape == (n_classes, 2) and not a.class_stats().any()
    x1, u1, s1 = _solve(a, batch)
    cold_order = a.last_queue_order()
    labels = a.instance_classes()
    stats = a.class_stats()
    assert stats.dtype == np.uint64
    np.testing.assert_array_equal(stats, _history(labels, s1["iters"], n_classes))
    np.testing.assert_array_equal(a.class_stats(5, 40), stats[5:45])
    _solve(a, batch)
    warm_order = a.last_queue_order()
    assert (warm_order != cold_order).any()                                # the history does reorder this queue
    c = DdpEngine("srbd13", N, B, opts=QUEUE3)                             # a fresh handle, seeded: its FIRST launch is A's second
    c.enable_auto_classes()
    c.add_class_stats(stats)
    np.testing.assert_array_equal(c.class_stats(), stats)
    xc, uc, sc = _solve(c, batch)
    np.testing.assert_array_equal(c.last_queue_order(), warm_order)
    np.testing.assert_array_equal(xc, x1); np.testing.assert_array_equal(uc, u1)
    np.testing.assert_array_equal(c.class_stats(), 2 * stats)              # ... and it goes on learning
    d = DdpEngine("srbd13", N, 4, opts=QUEUE3)                             # sums and counts are additive
    d.enable_auto_classes()
    d.add_class_stats(stats)
    d.add_class_stats(stats)
    np.testing.assert_array_equal(d.class_stats(), 2 * stats)
    d.add_class_stats(stats[7:9], first_class=7)                           # a range of classes
    want = 2 * stats
    want[7:9] += stats[7:9]
    np.testing.assert_array_equal(d.class_stats(), want)
    for e in (a, c, d):
        e.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_switching_off():
    N, B = 30, 6
    batch = workload.make_batch("srbd13", N, np.arange(B) + 100)
    labels, n_classes = workload.schedule_classes("srbd13", batch["params"])
    eng = DdpEngine("srbd13", N, B, opts=dict(OPTS, max_iters=0))
    for call in (eng.instance_classes, eng.class_stats, lambda: eng.device_buffer(12), lambda: eng.add_class_stats(np.zeros((1, 2), np.uint64))):
        with pytest.raises(RuntimeError):                                  # no class table yet
            call()
    eng.set_instance_classes(np.zeros(B, np.int32), 7)                     # caller labels first, another n_classes
    with pytest.raises(RuntimeError):
        eng.enable_auto_classes()
    assert eng.auto_classes_info() == (False, 7)
    eng.close()

    eng = DdpEngine("srbd13", N, B, opts=dict(OPTS, max_iters=0))
    eng.set_instance_classes(np.zeros(B, np.int32), n_classes)             # ... with the library's n_classes: the table is taken over
    eng.enable_auto_classes()
    with pytest.raises(RuntimeError):
        eng.set_instance_classes(labels, n_classes)
    with pytest.raises(RuntimeError):
        eng.set_instance_classes_range_device(0, B, _dev(labels, torch.int32), n_classes)
    _solve(eng, batch)
    np.testing.assert_array_equal(eng.instance_classes(), labels)
    stats = eng.class_stats()
    assert int(stats[:, 1].sum()) == B
    for first_class, count in ((n_classes, 1), (-1, 1), (n_classes - 1, 2), (0, 0)):
        with pytest.raises(RuntimeError):
            eng.class_stats(first_class, count)
    with pytest.raises(RuntimeError):
        eng.add_class_stats(np.zeros((2, 2), np.uint64), first_class=n_classes - 1)
    with pytest.raises(RuntimeError):
        eng.instance_classes(B - 1, 2)
    eng.enable_auto_classes(False)                                         # the labelling stops; labels and history stay
    assert eng.auto_classes_info() == (False, n_classes)
    np.testing.assert_array_equal(eng.instance_classes(), labels)
    np.testing.assert_array_equal(eng.class_stats(), stats)
    other = dict(batch, params=np.array(batch["params"]))
    other["params"][:, :, 17:19] = 0.0
    assert (workload.schedule_classes("srbd13", other["params"])[0] != labels).any()
    _solve(eng, other)
    np.testing.assert_array_equal(eng.instance_classes(), labels)         # not relabelled
    assert int(eng.class_stats()[:, 1].sum()) == 2 * B                     # still learning, under the labels it holds
    eng.set_instance_classes(labels[::-1].copy(), n_classes)               # and the caller may label again
    np.testing.assert_array_equal(eng.instance_classes(), labels[::-1])
    eng.close()


# ---- 7. the fleet queue -----------------------------------------------------------------------------------------------------------
def test_fleet_queue_needs_no_labels_on_a_handle_with_auto_classes():
    N, B, D = 30, 16, 2
    eng = DdpEngine("srbd13", N, D * B, opts=dict(OPTS, max_iters=0, max_slots=8, queue_order=3))
    eng.enable_auto_classes()
    blocks = [workload.make_batch("srbd13", N, np.arange(B) + 100 + 50 * i) for i in range(D)]
    fleet = FleetQueue(eng, torch.zeros((D * B, N + 1, 19), dtype=torch.float64, device="cuda"), B, D)
    for b in blocks:
        fleet.submit(_dev(b["x0"]), _dev(b["xs"]), _dev(b["us"]), params=_dev(b["params"]))      # classes=None
    assert fleet.flush() == D * B
    want = np.concatenate([workload.schedule_classes("srbd13", b["params"])[0] for b in blocks])
    np.testing.assert_array_equal(eng.instance_classes(), want)
    assert eng.queue_info()[1:] == (8, D * B)
    eng.close()
