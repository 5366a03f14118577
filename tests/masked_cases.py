"""Masked launches (include/sddp.h sddp_*_masked_device): what tests/test_masked_cpu.py and tests/test_gpu_masked.py share -- the
masks, and a numpy statement of the pre-pass that builds the queue of a masked launch (csrc/sddp_kernels_host.hpp): for each queue
order the partition, the order of the tail up to ties, the queue start.  No device here."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
B = 48                                                  # the batch of the GPU cases
SHAPES = {"srbd13": 10, "lip30": 8}                     # model -> N: a one-wave and a four-wave build at the horizons of tests/resume_cases.py


def mask_half(count, seed=7):
    """a fixed pseudo-random mask of about half of `count` instances, as int32 with other non-zero words than 1 among the selected"""
    r = np.random.default_rng(seed)
    m = (r.random(count) < 0.5).astype(np.int32)
    m[m != 0] = r.choice(np.array([1, 2, -1, 1 << 30], dtype=np.int32), int(m.sum()))
    return m


def edge_masks(count):
    """name -> mask: nothing, everything, the first instance of the range alone, the last alone"""
    only = lambda i: np.eye(1, count, i, dtype=np.int32)[0]      # noqa: E731
    return {"none": np.zeros(count, np.int32), "all": np.ones(count, np.int32), "first": only(0), "last": only(count - 1)}


def class_key(cost, cls, cls_stat):
    """queue order 3: class_key_kernel -- the class mean (1e6: unlabelled, or no history), the cost breaking ties"""
    cost = np.asarray(cost, dtype=np.float64)
    n_cls = len(cls_stat)
    mean = np.full(len(cost), 1e6)
    for i, c in enumerate(cls):
        if 0 <= c < n_cls and cls_stat[c][1] > 0:
            mean[i] = float(cls_stat[c][0]) / float(cls_stat[c][1])
    with np.errstate(invalid="ignore", over="ignore"):
        fin = (cost == cost) & (cost < 1e300)
        return np.where(fin, mean + 1e-3 * cost / (np.abs(cost) + 1e9), cost)


def keys(queue_order, count, hist=None, cost=None, cls=None, cls_stat=None):
    """the key every SELECTED instance of the range is handed out by, larger first; equal keys: any order.
    0: index order.  1: the previous iteration count, capped at 256, never solved (-1) first.  2: the initial cost, a NaN or an
    infinite one first (DBL_MAX after the clamp into the finite doubles).  3: the class key, clamped likewise; without a class table
    it is order 2."""
    if queue_order == 0:
        return -np.arange(count, dtype=np.float64)
    if queue_order == 1:
        h = np.asarray(hist)
        return np.where(h < 0, 257, np.minimum(h, 256)).astype(np.float64)
    k = np.asarray(cost, dtype=np.float64)
    k = np.where(k == k, k, np.inf)                                         # (the key kernel: a NaN start sorts first)
    if queue_order == 3 and cls is not None:
        k = class_key(k, cls, cls_stat)
    return np.where(k == k, np.clip(k, -DBL_MAX, DBL_MAX), DBL_MAX)


def prepass(mask, first, key):
    """-> (n_selected, queue start, the unselected instances as a set, the tail as a list of sets: the groups of equal key in the
    order the queue hands them out).  Instance indices are absolute (first + i)."""
    mask = np.asarray(mask)
    sel = np.flatnonzero(mask != 0)
    uns = set((first + np.flatnonzero(mask == 0)).tolist())
    groups = []
    for k in sorted(set(np.asarray(key)[sel].tolist()), reverse=True):
        groups.append(set((first + sel[np.asarray(key)[sel] == k]).tolist()))
    return len(sel), len(mask) - len(sel), uns, groups


def check_prepass(order, selected_words, mask, first, key):
    """the device's order array [count] and its two SDDP_BUF_SELECTED words against the statement above"""
    n, start, uns, groups = prepass(mask, first, key)
    order = np.asarray(order).tolist()
    assert list(selected_words) == [n, start], (selected_words, n, start)
    assert len(order) == len(mask)
    assert set(order[:start]) == uns and len(set(order)) == len(order), "the partition is not exact"
    at = start
    for g in groups:
        assert set(order[at:at + len(g)]) == g, f"tail position {at}: {order[at:at + len(g)]} is not the group {sorted(g)}"
        at += len(g)
    assert at == len(order)
