"""The class label that a handle computes itself (include/sddp.h sddp_enable_auto_classes), without a device: the numpy statement
workload.schedule_classes against the labels written down with the hand-built cases (tests/auto_class_cases.py) and against
srbd13_schedule_classes, which bench.py passes today; the columns of the other three models."""
import os
import re

import numpy as np
import pytest

from srbd_horizon_amd import workload
from tests import auto_class_cases as acc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,B", [(30, 37), (70, 37), (8, 8)])
def test_srbd13_labels_of_the_hand_built_cases(N, B):
    c = acc.build("srbd13", N, B)
    assert B == 8 or B >= len(acc.cases(N))                       # every case is some instance's
    labels, n = workload.schedule_classes("srbd13", c["params"])
    assert labels.dtype == np.int32 and n == c["n_classes"] == 36 * (N + 2)
    np.testing.assert_array_equal(labels, c["labels"])
    old, n_old = workload.srbd13_schedule_classes(c["params"])
    assert n_old == n
    np.testing.assert_array_equal(labels, old)
    assert labels.min() >= 0 and labels.max() < n


def test_the_cases_cover_what_they_claim():
    for N in (30, 70):
        c = acc.build("srbd13", N, 37)
        assert set(c["stance0"].tolist()) == {0, 1, 2, 3}
        want = {1, 2, N - 1, N, N + 1} | ({63, 64, 65} if N + 1 > 64 else set())
        assert want <= set(c["first_change"].tolist())
        P = c["params"]
        assert np.isnan(P[:, 0, 17]).any() and np.isnan(P[:, 1:, 17:19]).any() and (P[:, :, 17:19] == 0.5).any()
        for col in (0, 1):
            got = {(float(v), bool(np.signbit(v))) for v in P[:, N, col]}
            assert got == {(float(v), bool(np.signbit(v))) for v in acc.CMDS}


@pytest.mark.parametrize("seed0", [0, 100, 4000])
def test_srbd13_labels_of_generated_batches_equal_the_callers_function(seed0):
    for N in (30, 12):
        P = workload.make_batch("srbd13", N, np.arange(64) + seed0)["params"]
        new, n_new = workload.schedule_classes("srbd13", P)
        old, n_old = workload.srbd13_schedule_classes(P)
        assert n_new == n_old == 36 * (N + 2)
        np.testing.assert_array_equal(new, old)
        assert len(np.unique(new)) >= 6


@pytest.mark.parametrize("model", ["srbd37", "lip30", "srbd61"])
def test_the_other_models_labels_follow_from_their_columns(model):
    N, B = 8, 8
    c = acc.build(model, N, B)
    assert c["params"].shape[2] == _lib_dims(model)
    labels, n = workload.schedule_classes(model, c["params"])
    assert n == 36 * (N + 2)
    np.testing.assert_array_equal(labels, c["labels"])
    np.testing.assert_array_equal(labels, acc.build("srbd13", N, B)["labels"])      # the same schedule, the same label
    # the generated batches of all models share schedule and command per seed: so do their labels, read from each model's columns
    seeds = np.arange(48) + 7
    ref, _ = workload.srbd13_schedule_classes(workload.make_batch("srbd13", 20, seeds)["params"])
    got, _ = workload.schedule_classes(model, workload.make_batch(model, 20, seeds)["params"])
    np.testing.assert_array_equal(got, ref)
    assert len(np.unique(ref)) >= 6


def _lib_dims(model):
    return {"srbd13": 19, "srbd37": 19, "lip30": 11, "srbd61": 27}[model]


def test_reference_columns_of_user_rows_are_not_read():
    c, cx = acc.build("srbd13", 30, 37), acc.build("srbd13", 30, 37, 8)
    assert cx["params"].shape[2] == 19 + 8
    np.testing.assert_array_equal(workload.schedule_classes("srbd13", cx["params"])[0], c["labels"])


def test_the_columns_are_the_device_models():
    """csrc/sddp_models.hpp states the columns as P_CMD0 / P_CMD1 / P_SW_L / P_SW_R of each model; here as numbers"""
    assert workload.CLASS_COLUMNS == {"srbd13": dict(cmd=(0, 1), sw=(17, 18)), "srbd37": dict(cmd=(0, 1), sw=(8, 12)),
                                      "srbd61": dict(cmd=(0, 1), sw=(8, 16)), "lip30": dict(cmd=(0, 1), sw=(4, 8))}
    src = open(os.path.join(ROOT, "srbd_horizon_amd", "csrc", "sddp_models.hpp")).read()
    assert len(re.findall(r"\bP_SW_L\b", src)) >= 2 and len(re.findall(r"\bP_SW_R\b", src)) >= 2       # SRBD family and LIP

