"""The life cycle of a handle's optional buffer groups (csrc/sddp_handle.hpp: resume, iteration log, policy, class history,
instance table, cold queue): switched on, used, switched off in reverse order, switched on again with other sizes -- and after
every step the handle solves to the bytes of a plain handle and its reporting calls say what was just set.

That each feature alone changes no bit is established by its own module (tests/test_gpu_resume.py, test_gpu_iteration_log.py,
test_gpu_deadline.py, test_gpu_policy.py, test_gpu_auto_classes.py, test_gpu_instance_consts.py); this one asserts that allocating,
giving up and re-allocating the groups on one handle does not either.  One handle per kernel family, at the smallest shape that
has a work queue and its ordering buffers in play: N = 4, B = 6 on max_slots = 2."""
import functools

import numpy as np
import pytest

from srbd_horizon_amd.engine import DdpEngine
from tests import oracle_refs as refs
from tests.gpu_support import frozen, same_bytes, solve

pytestmark = pytest.mark.gpu

N, B, SLOTS = 4, 6, 2
OPTS = dict(max_iters=20, max_slots=SLOTS)
NEVER = 60e6                                                     # microseconds: a budget that never runs out
FAMILIES = [("srbd13", 1, 1), ("srbd13", 2, 1), ("srbd61", 1, 4)]      # model, waves_per_simd, wavefronts per instance
N_CLASSES = 36 * (N + 2)                                         # the library's own labels (sddp_enable_auto_classes)


@functools.lru_cache(maxsize=None)
def batch(model):
    return refs.batch(model, N, range(B))


def engine(model, wps):
    return DdpEngine(model, N, B, opts=dict(OPTS, waves_per_simd=wps), consts=batch(model)["consts"])


@functools.lru_cache(maxsize=None)
def reference(model, wps):
    """a fresh plain handle of the same shape, solved once: read-only"""
    eng = engine(model, wps)
    out = solve(eng, batch(model))
    eng.close()
    return frozen(out)


def refused(call, text):
    with pytest.raises(RuntimeError, match=text):
        call()


def reports(eng, resume, rows, budget, knots, auto, table):
    """the reporting calls say exactly this; a group that is off refuses what only it can answer"""
    if resume is None:
        refused(eng.unfinished, "sddp_enable_resume has not been called")
    else:
        assert eng.unfinished() == resume
    assert eng.iteration_log_rows() == rows
    assert eng.time_budget() == budget
    if knots == 0:
        refused(eng.policy_words, "sddp_enable_policy has not been called")
    else:
        assert eng.policy_words() == (knots * eng.nu * (eng.nx + 1) + 4, knots)
    assert eng.auto_classes_info() == auto
    assert eng.instance_consts_active() == table


def everything_on(eng, rows, knots):
    """every group, in the order a caller has to respect (the log and the budget ride on resume); the reports follow each step"""
    had_classes = eng.auto_classes_info()[1]                     # the class table outlives enable_auto_classes(False)
    eng.enable_resume()
    reports(eng, 0, 0, (0.0, 0), 0, (False, had_classes), False)
    eng.enable_iteration_log(rows)
    reports(eng, 0, rows, (0.0, 0), 0, (False, had_classes), False)
    eng.set_time_budget(NEVER, 0)
    reports(eng, 0, rows, (NEVER, 0), 0, (False, had_classes), False)
    eng.enable_policy(knots)
    reports(eng, 0, rows, (NEVER, 0), knots, (False, had_classes), False)
    eng.set_options(queue_order=3)
    eng.enable_auto_classes()
    reports(eng, 0, rows, (NEVER, 0), knots, (True, N_CLASSES), False)
    eng.set_instance_consts({"m": np.full(B, eng.consts.m)})    # every row: the handle's own constants
    reports(eng, 0, rows, (NEVER, 0), knots, (True, N_CLASSES), True)


def solves_like(eng, ref, model, msg):
    same_bytes(solve(eng, batch(model)), ref, msg=msg)
    assert eng.queue_info() == (SLOTS, SLOTS, B)                 # two slots pull six instances from the queue


@pytest.mark.parametrize("model,wps,waves", FAMILIES)
def test_groups_switched_on_off_and_on_again_change_no_bit_and_report_their_state(model, wps, waves):
    ref = reference(model, wps)
    open_ = int((ref[2]["status"] == 1).sum())                   # what the solve itself leaves at max_iters: nothing is cut by time
    eng = engine(model, wps)
    assert eng.queue_info() == (SLOTS, 0, 0)
    solves_like(eng, ref, model, "(plain)")
    assert eng.kernel_info()["wavefronts_per_instance"] == waves
    reports(eng, None, 0, (0.0, 0), 0, (False, 0), False)

    everything_on(eng, 4, 2)
    solves_like(eng, ref, model, "(everything on)")
    eng.policy_range_device()
    assert eng.fetch_policy().shape == (B, eng.policy_words()[0])
    rec, n = eng.iteration_log()
    assert rec.shape == (B, 4, 16) and n.shape == (B,)
    assert (eng.instance_classes() >= 0).all()                   # the solve labelled every instance
    reports(eng, open_, 4, (NEVER, 0), 2, (True, N_CLASSES), True)

    # off, in reverse order
    eng.clear_instance_consts()
    reports(eng, 0, 4, (NEVER, 0), 2, (True, N_CLASSES), False)  # (the rewritten rows cannot be continued: the flags are cleared)
    eng.enable_auto_classes(False)
    eng.set_options(queue_order=1)
    reports(eng, 0, 4, (NEVER, 0), 2, (False, N_CLASSES), False)
    eng.enable_policy(0)
    reports(eng, 0, 4, (NEVER, 0), 0, (False, N_CLASSES), False)
    eng.set_time_budget(0.0)
    reports(eng, 0, 4, (0.0, 0), 0, (False, N_CLASSES), False)
    eng.enable_iteration_log(0)
    reports(eng, 0, 0, (0.0, 0), 0, (False, N_CLASSES), False)
    eng.enable_resume(False)
    reports(eng, None, 0, (0.0, 0), 0, (False, N_CLASSES), False)
    solves_like(eng, ref, model, "(everything off again)")

    # on again, with other sizes
    everything_on(eng, 8, 1)
    solves_like(eng, ref, model, "(on again: log rows 8, policy knots 1)")
    assert eng.iteration_log()[0].shape == (B, 8, 16)
    reports(eng, open_, 8, (NEVER, 0), 1, (True, N_CLASSES), True)

    # resume off takes the log and the budget with it; the other groups stay
    eng.enable_resume(False)
    reports(eng, None, 0, (0.0, 0), 1, (True, N_CLASSES), True)
    refused(eng.continue_solve, "sddp_enable_resume has not been called")
    refused(lambda: eng.enable_iteration_log(4), "call sddp_enable_resume first")
    refused(lambda: eng.set_time_budget(NEVER), "call sddp_enable_resume first")
    solves_like(eng, ref, model, "(resume off, the rest on)")
    eng.close()
