"""Masked launches without a device: the numpy statement of the pre-pass (tests/masked_cases.py) accepts what the contract allows
and refuses what it forbids, for every queue order; the binding and the argument checks of the Python face."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from srbd_horizon_amd import _lib
from srbd_horizon_amd.engine import DdpEngine
from tests import abi_header, masked_cases as mc

COUNT, FIRST = 37, 5


def _inputs(seed=3):
    r = np.random.default_rng(seed)
    hist = r.integers(-1, 7, COUNT)
    hist[3] = 1000                                                          # above the cap: bin 256, with every other count > 256
    hist[4] = 300
    cost = r.random(COUNT) * 1e3
    cls = r.integers(-1, 4, COUNT)
    cls_stat = np.array([[30, 3], [0, 0], [45, 5], [7, 1]], dtype=np.uint64)   # class 1: no history
    return hist, cost, cls, cls_stat


def _a_right_order(mask, key, rng):
    """one order the contract allows: the unselected instances shuffled, the selected ones by descending key, ties shuffled"""
    sel, uns = np.flatnonzero(mask != 0), np.flatnonzero(mask == 0)
    sel = sel[rng.permutation(len(sel))]
    tail = sel[np.argsort(-np.asarray(key)[sel], kind="stable")]
    return FIRST + np.concatenate([uns[rng.permutation(len(uns))], tail])


@pytest.mark.parametrize("queue_order", [0, 1, 2, 3])
def test_the_statement_of_the_pre_pass(queue_order):
    hist, cost, cls, cls_stat = _inputs()
    mask = mc.mask_half(COUNT)
    assert 0 < np.count_nonzero(mask) < COUNT and set(np.unique(mask)) - {0, 1}     # words other than 0 / 1 select as well
    sel = np.flatnonzero(mask)
    cost[sel[0]], cost[sel[1]], cost[sel[2]] = np.nan, np.inf, -np.inf              # bad keys among the selected
    key = mc.keys(queue_order, COUNT, hist, cost, cls, cls_stat)
    assert np.all(np.isfinite(key))                                                 # no selected key can tie with an unselected +inf
    rng = np.random.default_rng(11)
    n, start, uns, groups = mc.prepass(mask, FIRST, key)
    assert (n, start) == (len(sel), COUNT - len(sel)) and sum(map(len, groups)) == n and len(uns) == start
    for _ in range(4):
        order = _a_right_order(mask, key, rng)
        mc.check_prepass(order, (n, start), mask, FIRST, key)
    if queue_order >= 2:                                                            # the NaN and the +inf start lead the tail, behind every unselected one
        assert set(order[start:start + 2]) == {FIRST + sel[0], FIRST + sel[1]}
    if queue_order == 2:
        assert order[-1] == FIRST + sel[2]
    if queue_order == 1:
        assert key[3] == key[4] == 256
    # refused: a selected instance in front of the queue start, a wrong count, a tail out of order, a duplicate
    bad = order.copy()
    bad[0], bad[start] = bad[start], bad[0]
    with pytest.raises(AssertionError):
        mc.check_prepass(bad, (n, start), mask, FIRST, key)
    with pytest.raises(AssertionError):
        mc.check_prepass(order, (n + 1, start - 1), mask, FIRST, key)
    if len(groups) > 1:
        bad = order.copy()
        i, j = start, start + len(groups[0])                                        # the first of two different groups, swapped
        bad[i], bad[j] = bad[j], bad[i]
        with pytest.raises(AssertionError):
            mc.check_prepass(bad, (n, start), mask, FIRST, key)
    bad = order.copy()
    bad[-1] = bad[-2]
    with pytest.raises(AssertionError):
        mc.check_prepass(bad, (n, start), mask, FIRST, key)


def test_edge_masks_of_the_statement():
    key = mc.keys(0, COUNT)
    for name, m in mc.edge_masks(COUNT).items():
        n, start, uns, groups = mc.prepass(m, FIRST, key)
        assert n == {"none": 0, "all": COUNT, "first": 1, "last": 1}[name] and start == COUNT - n
        assert [min(g) for g in groups] == sorted(FIRST + np.flatnonzero(m))        # index order, one instance per group
    assert mc.prepass(np.ones(1, np.int32), 9, mc.keys(0, 1)) == (1, 0, set(), [{9}])


def test_class_keys_are_the_kernels_formula():
    cost = np.array([10.0, 20.0, np.inf, 5.0, 1e301])
    k = mc.class_key(cost, [0, 0, 0, -1, 2], np.array([[30, 3], [0, 0], [45, 5]], dtype=np.uint64))
    assert k[0] < k[1] and abs(k[0] - 10.0) < 1e-3 and k[2] == np.inf and abs(k[3] - 1e6) < 1e-3 and k[4] == 1e301


def test_the_binding_of_the_masked_entry_points():
    vp, i = C.c_void_p, C.c_int
    want = {"sddp_solve_masked_device": [vp, vp, i, i, vp], "sddp_continue_masked_device": [vp, vp, i, i, vp],
            "sddp_policy_masked_device": [vp, i, i, vp], "sddp_advance_masked_device": [vp, i, i, vp, vp, vp],
            "sddp_last_selected": [vp, C.POINTER(i)]}
    declared = abi_header.functions()
    for name, args in want.items():
        assert _lib.SYMBOLS[name] == (i, args) and name in declared
        assert len(declared[name][1]) == len(args)
    assert _lib.DEVICE_BUF_SELECTED == 14 == _lib.DEVICE_BUF_VALUE + 1
    assert re.search(r"^#define\s+SDDP_BUF_SELECTED\s+\(SDDP_BUF_CLASSES \+ 2\)", abi_header.text(), flags=re.M)
    for name in ("solve_masked_device", "continue_masked", "policy_masked_device", "advance_masked_device", "last_selected"):
        assert callable(getattr(DdpEngine, name))


def test_a_mask_is_checked_before_the_library_sees_it():
    for bad in (np.ones(4, np.int32), torch.ones(4, dtype=torch.int32), [1, 0, 1, 1], None):     # no device tensor
        with pytest.raises(ValueError, match="int32 CUDA tensor"):
            DdpEngine._mask(bad, 4)
