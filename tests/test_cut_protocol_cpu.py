"""The cut-and-continue launch sequence of the Python layer (resumable solves, include/sddp.h), call for call: what
FleetQueue.solve_sliced / solve_within and DDPSolver.set_slices / set_time_budget / _launch ask of the engine, in which order and
with which arguments, and how they leave it.  No GPU and no library: a recording stand-in takes the calls, its `unfinished` is
scripted.  The expected logs are the sequences of the first implementation (four hand-written copies), written down before the
copies were folded into DdpEngine.cut_and_continue."""
import types

import numpy as np
import pytest
import torch

from srbd_horizon_amd import _lib
from srbd_horizon_amd.ddp import DDPSolver
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.fleet import FleetQueue

N, NX, NU, NP, WORDS = 4, 3, 2, 5, 4
OVERRUN = 12.5


class RecordingEngine(DdpEngine):
    """DdpEngine without a handle: every state-changing or launching call is appended to `log` with its arguments (device
    tensors by what identifies them: `params` by whether one was passed, a record buffer by the order of its first appearance);
    `unfinished` answers from the script.  The getters are not logged.  Whatever DdpEngine builds on these calls is the real code."""

    def __init__(self, B, max_iters=50, unfinished=(), resume=False, budget=(0.0, 0)):
        self.h = None
        self.B, self.N, self.nx, self.nu, self.np_ = B, N, NX, NU, NP
        self.opts = types.SimpleNamespace(max_iters=max_iters)
        self.resume_enabled, self.budget = resume, budget
        self.script, self.log, self.bufs = list(unfinished), [], {}
        self.stats = np.zeros(B, dtype=_lib.STATS_DTYPE)
        self.si = torch.from_numpy(self.stats.view(np.int32).reshape(B, _lib.STATS_I32_WORDS))

    # ---- logged ----
    def enable_resume(self, on=True):
        self.log.append(("enable_resume", bool(on)))
        self.resume_enabled = bool(on)
        if not on:
            self.budget = (0.0, 0)                       # sddp_enable_resume(h, 0) disarms the budget

    def set_options(self, **over):
        self.log.append(("set_options", dict(over)))
        for k, v in over.items():
            setattr(self.opts, k, v)

    def set_time_budget(self, budget_us, min_iters=0):
        assert self.resume_enabled or budget_us == 0.0, "the library refuses a budget without resumable solves"
        self.log.append(("set_time_budget", float(budget_us), int(min_iters)))
        self.budget = (float(budget_us), int(min_iters) if budget_us > 0.0 else 0)

    def _ran(self, what, first, count):
        self.log.append(what)
        self.si[first:first + count, _lib.STATS_I32_STATUS] = 0
        if self.script:                                  # the instances the next `unfinished` will report are left at status 1
            self.si[first:first + self.script[0], _lib.STATS_I32_STATUS] = 1

    def solve_range_device(self, params, first, count):
        self._ran(("solve_range_device", params is not None, int(first), int(count)), first, count)

    def solve(self, params):
        self._ran(("solve",), 0, self.B)
        return np.full((self.B, N + 1, NX), 1.0), np.full((self.B, N, NU), 1.0)

    def solve_resident(self):
        self._ran(("solve_resident",), 0, self.B)
        return np.full((self.B, N + 1, NX), 1.0), np.full((self.B, N, NU), 1.0)

    def continue_solve(self, params=None, first=0, count=None):
        assert self.resume_enabled
        self.log.append(("continue_solve", params is not None, first, count))

    def pack_records_device(self, out, first, count, mode="full"):
        self.log.append(("pack_records_device", self.bufs.setdefault(out.data_ptr(), len(self.bufs)), tuple(out.shape), first, count, mode))
        return out

    def unfinished(self, first=0, count=None):
        assert self.resume_enabled
        self.log.append(("unfinished", first, count))
        return self.script.pop(0)

    def deadline_overrun_us(self):
        self.log.append(("deadline_overrun_us",))
        return OVERRUN

    # ---- not logged ----
    def record_words(self, mode="full"):
        return WORDS

    def time_budget(self):
        return self.budget

    def fetch(self):
        return np.full((self.B, N + 1, NX), 2.0), np.full((self.B, N, NU), 2.0), self.stats

    def fetch_device_views(self):
        z = lambda *s: torch.zeros(s, dtype=torch.float64)
        return z(self.B, N + 1, NX), z(self.B, N, NU), z(self.B, _lib.STATS_F64_WORDS), self.si

    def load_range_device(self, first, count, x0=None, x=None, u=None):
        pass


def queue(**kw):
    """a queue of depth 2 over batches of 2 with ONE batch pending: the launches cover the instances [0, 2) of 4"""
    eng = RecordingEngine(4, **kw)
    q = FleetQueue(eng, torch.zeros(4, N + 1, NP, dtype=torch.float64), 2, 2)
    q.submit(None, None, None)
    return eng, q


def left_as_found(eng, resume, budget=(0.0, 0)):
    return (eng.resume_enabled, eng.budget, eng.opts.max_iters) == (resume, budget, 50)


# ---- FleetQueue.solve_sliced -----------------------------------------------------------------------------------------------------
def test_solve_sliced_resume_off_all_finished():
    eng, q = queue(unfinished=[0])
    finished, records = q.solve_sliced(3, 100)
    assert eng.log == [("enable_resume", True),
                       ("set_options", {"max_iters": 3}),
                       ("solve_range_device", True, 0, 2),
                       ("pack_records_device", 0, (2, WORDS), 0, 2, "first_knot"),
                       ("set_options", {"max_iters": 100}),
                       ("unfinished", 0, 2),
                       ("enable_resume", False),
                       ("set_options", {"max_iters": 50})]
    assert finished.tolist() == [True, True] and records is q.first_records
    assert (q.launches, q.pending) == (1, 0) and left_as_found(eng, False)


def test_solve_sliced_resume_off_one_unfinished():
    eng, q = queue(unfinished=[1])
    finished, records = q.solve_sliced(3, 100)
    assert eng.log == [("enable_resume", True),
                       ("set_options", {"max_iters": 3}),
                       ("solve_range_device", True, 0, 2),
                       ("pack_records_device", 0, (2, WORDS), 0, 2, "first_knot"),
                       ("set_options", {"max_iters": 100}),
                       ("unfinished", 0, 2),
                       ("continue_solve", True, 0, 2),
                       ("pack_records_device", 1, (2, WORDS), 0, 2, "first_knot"),
                       ("enable_resume", False),
                       ("set_options", {"max_iters": 50})]
    assert finished.tolist() == [False, True] and records is not q.first_records
    assert (q.launches, q.pending) == (2, 0) and left_as_found(eng, False)


def test_solve_sliced_resume_on_all_finished():
    eng, q = queue(unfinished=[0], resume=True)
    finished, records = q.solve_sliced(3, 100)
    assert eng.log == [("enable_resume", True),
                       ("set_options", {"max_iters": 3}),
                       ("solve_range_device", True, 0, 2),
                       ("pack_records_device", 0, (2, WORDS), 0, 2, "first_knot"),
                       ("set_options", {"max_iters": 100}),
                       ("unfinished", 0, 2),
                       ("set_options", {"max_iters": 50})]
    assert finished.tolist() == [True, True] and records is q.first_records
    assert (q.launches, q.pending) == (1, 0) and left_as_found(eng, True)


def test_solve_sliced_resume_on_two_unfinished_twice():
    """the second call reuses the two record buffers of the first"""
    eng, q = queue(unfinished=[2, 2], resume=True)
    q.solve_sliced(3, 100)
    q.submit(None, None, None)
    del eng.log[:]
    finished, records = q.solve_sliced(3, 100)
    assert eng.log == [("enable_resume", True),
                       ("set_options", {"max_iters": 3}),
                       ("solve_range_device", True, 0, 2),
                       ("pack_records_device", 0, (2, WORDS), 0, 2, "first_knot"),
                       ("set_options", {"max_iters": 100}),
                       ("unfinished", 0, 2),
                       ("continue_solve", True, 0, 2),
                       ("pack_records_device", 1, (2, WORDS), 0, 2, "first_knot"),
                       ("set_options", {"max_iters": 50})]
    assert finished.tolist() == [False, False] and records is not q.first_records
    assert (q.launches, q.pending) == (4, 0) and left_as_found(eng, True)


# ---- FleetQueue.solve_within -----------------------------------------------------------------------------------------------------
def test_solve_within_resume_off_all_finished():
    eng, q = queue(unfinished=[0])
    finished, records = q.solve_within(250.0, 100, 1)
    assert eng.log == [("enable_resume", True),
                       ("set_options", {"max_iters": 100}),
                       ("set_time_budget", 250.0, 1),
                       ("solve_range_device", True, 0, 2),
                       ("pack_records_device", 0, (2, WORDS), 0, 2, "first_knot"),
                       ("set_time_budget", 0.0, 0),
                       ("unfinished", 0, 2),
                       ("deadline_overrun_us",),
                       ("enable_resume", False),
                       ("set_options", {"max_iters": 50})]
    assert finished.tolist() == [True, True] and records is q.first_records and q.overrun_us == OVERRUN
    assert (q.launches, q.pending) == (1, 0) and left_as_found(eng, False)


def test_solve_within_resume_off_one_unfinished():
    eng, q = queue(unfinished=[1])
    finished, records = q.solve_within(250.0, 100)
    assert eng.log == [("enable_resume", True),
                       ("set_options", {"max_iters": 100}),
                       ("set_time_budget", 250.0, 0),
                       ("solve_range_device", True, 0, 2),
                       ("pack_records_device", 0, (2, WORDS), 0, 2, "first_knot"),
                       ("set_time_budget", 0.0, 0),
                       ("unfinished", 0, 2),
                       ("deadline_overrun_us",),
                       ("continue_solve", True, 0, 2),
                       ("pack_records_device", 1, (2, WORDS), 0, 2, "first_knot"),
                       ("enable_resume", False),
                       ("set_options", {"max_iters": 50})]
    assert finished.tolist() == [False, True] and records is not q.first_records and q.overrun_us == OVERRUN
    assert (q.launches, q.pending) == (2, 0) and left_as_found(eng, False)


def test_solve_within_resume_on_all_finished():
    eng, q = queue(unfinished=[0], resume=True)
    finished, records = q.solve_within(250.0, 100, 1)
    assert eng.log == [("enable_resume", True),
                       ("set_options", {"max_iters": 100}),
                       ("set_time_budget", 250.0, 1),
                       ("solve_range_device", True, 0, 2),
                       ("pack_records_device", 0, (2, WORDS), 0, 2, "first_knot"),
                       ("set_time_budget", 0.0, 0),
                       ("unfinished", 0, 2),
                       ("deadline_overrun_us",),
                       ("set_time_budget", 0.0, 0),
                       ("set_options", {"max_iters": 50})]
    assert finished.tolist() == [True, True] and records is q.first_records
    assert (q.launches, q.pending) == (1, 0) and left_as_found(eng, True)


def test_solve_within_resume_on_budget_armed_before_is_armed_again():
    eng, q = queue(unfinished=[2], resume=True, budget=(800.0, 3))
    finished, records = q.solve_within(250.0, 100, 1)
    assert eng.log == [("enable_resume", True),
                       ("set_options", {"max_iters": 100}),
                       ("set_time_budget", 250.0, 1),
                       ("solve_range_device", True, 0, 2),
                       ("pack_records_device", 0, (2, WORDS), 0, 2, "first_knot"),
                       ("set_time_budget", 0.0, 0),
                       ("unfinished", 0, 2),
                       ("deadline_overrun_us",),
                       ("continue_solve", True, 0, 2),
                       ("pack_records_device", 1, (2, WORDS), 0, 2, "first_knot"),
                       ("set_time_budget", 800.0, 3),
                       ("set_options", {"max_iters": 50})]
    assert finished.tolist() == [False, False] and records is not q.first_records
    assert (q.launches, q.pending) == (2, 0) and left_as_found(eng, True, (800.0, 3))


def test_an_empty_queue_makes_no_call():
    eng = RecordingEngine(4)
    q = FleetQueue(eng, torch.zeros(4, N + 1, NP, dtype=torch.float64), 2, 2)
    assert q.solve_sliced(3, 100) == (None, None) and q.solve_within(250.0, 100) == (None, None)
    assert eng.log == [] and (q.launches, q.pending) == (0, 0)


# ---- DDPSolver: set_slices, set_time_budget, _launch -----------------------------------------------------------------------------
def solver(**kw):
    """DDPSolver's launch state over the stand-in (the problem side of the adapter plays no part in it)"""
    s = object.__new__(DDPSolver)
    s.ddp_solver, s.slices = RecordingEngine(1, **kw), None
    return s.ddp_solver, s


def test_launch_in_slices_finished_by_the_first():
    eng, s = solver(unfinished=[0, 0])
    s.set_slices((2, 100))
    assert eng.log == [("enable_resume", True), ("set_options", {"max_iters": 100})]
    del eng.log[:]
    x, u = s._launch(lambda: eng.solve(None))
    assert eng.log == [("set_options", {"max_iters": 2}),
                       ("solve",),
                       ("set_options", {"max_iters": 100}),
                       ("unfinished", 0, None)]
    assert x[0, 0, 0] == 1.0 and u[0, 0, 0] == 1.0                    # what the first launch returned
    del eng.log[:]
    s._launch(eng.solve_resident)
    assert eng.log == [("set_options", {"max_iters": 2}),
                       ("solve_resident",),
                       ("set_options", {"max_iters": 100}),
                       ("unfinished", 0, None)]
    assert eng.resume_enabled and eng.opts.max_iters == 100
    del eng.log[:]
    s.set_slices(None)
    assert eng.log == [("enable_resume", False)] and s.slices is None


def test_launch_in_slices_continued():
    eng, s = solver(unfinished=[1])
    s.set_slices((2, 100))
    del eng.log[:]
    x, u = s._launch(lambda: eng.solve(None))
    assert eng.log == [("set_options", {"max_iters": 2}),
                       ("solve",),
                       ("set_options", {"max_iters": 100}),
                       ("unfinished", 0, None),
                       ("continue_solve", False, 0, None)]
    assert x[0, 0, 0] == 2.0 and u[0, 0, 0] == 2.0                    # what was fetched behind the continue launch
    assert eng.resume_enabled and eng.opts.max_iters == 100 and eng.budget == (0.0, 0)


def test_launch_without_slices_is_the_solve_alone():
    eng, s = solver()
    x, u = s._launch(lambda: eng.solve(None))
    assert eng.log == [("solve",)] and x[0, 0, 0] == 1.0


def test_time_budget_on_then_off_without_slices():
    eng, s = solver()
    s.set_time_budget(None)
    s.set_time_budget(0.0)
    assert eng.log == []                                              # nothing to switch off
    s.set_time_budget(500.0, 2)
    assert eng.log == [("enable_resume", True), ("set_time_budget", 500.0, 2)]
    del eng.log[:]
    s._launch(lambda: eng.solve(None))
    assert eng.log == [("solve",)]                                    # one launch, cut by the clock; nothing continues it
    del eng.log[:]
    s.set_time_budget(None)
    assert eng.log == [("set_time_budget", 0.0, 0), ("enable_resume", False)]
    assert not eng.resume_enabled and eng.budget == (0.0, 0)


def test_time_budget_with_slices_is_refused_and_off_leaves_the_slices():
    eng, s = solver()
    s.set_slices((2, 100))
    del eng.log[:]
    with pytest.raises(ValueError, match="a time budget and slices are two ways to cut a solve"):
        s.set_time_budget(500.0)
    assert eng.log == []
    s.set_time_budget(0.0)
    assert eng.log == [("set_time_budget", 0.0, 0)]
    assert eng.resume_enabled and s.slices == (2, 100)
