"""Every launcher of a model build through ONE handle (sddp_launch.hpp: solve in both register-file builds, policy export, backward
sweep, forward rollout, each without and with the constants table, the two instantiations of a kernel), checked bit for bit
against fresh handles.

A handle keeps per-kernel launch state (dynamic-LDS attribute, resident workgroups) from the first launch of each kernel on.  The
other tests drive one or two launchers per handle; here one handle meets every kernel of its build in turn, switches the constants
table on and off in between, and each step must leave exactly what a fresh handle leaves that performs only that step.  Two steps
cannot stand alone and carry their prerequisite on the fresh handle too: a policy launch needs a solve on the handle (it sweeps
against that launch's parameters and is refused without one), and a forward rollout applies the gains a backward sweep left.
x0 and both warm starts are uploaded again before every step, so each step starts from the same iterate.  No timing.
Options as in tests/test_gpu_divergence.py."""
import numpy as np
import pytest

from srbd_horizon_amd import workload
from srbd_horizon_amd.engine import DdpEngine

pytestmark = pytest.mark.gpu
OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)      # dsrbd_example.py:55-58
N, B = 4, 3
STEPS = ("solve_w1", "solve_w2", "policy", "backward", "forward")


def _load(eng, batch):
    eng.load(batch["x0"], batch["xs"], batch["us"])


def _info(eng):
    return eng.kernel_info(), eng.queue_info()


def _step(eng, batch, name):
    """One step on `eng` from the uploaded iterate -> (float arrays, raw records, kernel_info / queue_info or None)."""
    _load(eng, batch)
    if name in ("solve_w1", "solve_w2"):
        eng.set_options(waves_per_simd=1 if name == "solve_w1" else 2)
        x, u = eng.solve(batch["params"])
        return [x.copy(), u.copy()], eng.stats.tobytes(), _info(eng)
    if name == "policy":
        eng.policy_range_device()
        return [eng.fetch_policy()], b"", _info(eng)
    if name == "backward":
        kff, K, scal = eng.backward(batch["params"], mu=0.0)
        return [kff.copy(), K.copy(), scal.copy()], b"", None
    x, u, cost = eng.forward(batch["params"], 0.5)
    return [x.copy(), u.copy(), cost.copy()], b"", None


def _fresh(model, batch, name, masses):
    """What a fresh handle leaves that performs only step `name` (behind its prerequisite, see above)."""
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    if masses is not None:
        eng.set_instance_consts({"m": masses})
    if name == "policy":
        eng.enable_policy(1)
        _step(eng, batch, "solve_w2")
    if name == "forward":
        _step(eng, batch, "backward")
    out = _step(eng, batch, name)
    eng.close()
    return out


def _same(got, ref, what):
    assert len(got[0]) == len(ref[0])
    for a, r in zip(got[0], ref[0]):
        assert a.shape == r.shape and a.dtype == np.float64, what
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(r).view(np.uint64)), what
    assert got[1] == ref[1], what                     # the raw sddp_stats records
    if ref[2] is not None:
        assert got[2] == ref[2], (what, got[2], ref[2])
        assert got[2][0]["resources"]["workgroups_per_cu"] == ref[2][0]["resources"]["workgroups_per_cu"] >= 1


@pytest.mark.parametrize("model", ["srbd13", "lip30"])     # one wavefront per instance; four, with a half-register-file build
def test_one_handle_through_every_launcher_matches_fresh_handles(model):
    batch = workload.make_batch(model, N, np.arange(B) + 5)
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    masses = eng.consts.m * np.array([0.8, 1.0, 1.25])
    results = {}
    for het in (None, masses):
        if het is not None:
            eng.set_instance_consts({"m": het})
        assert eng.instance_consts_active() == (het is not None)
        last_solve = None
        for name in STEPS:
            if name == "policy":
                eng.enable_policy(1)
            got = _step(eng, batch, name)
            what = f"{model} {name} {'per-instance constants' if het is not None else 'handle constants'}"
            _same(got, _fresh(model, batch, name, het), what)
            if got[2] is None:
                assert _info(eng) == last_solve, what          # a phase-level launch is no solve launch
            else:
                last_solve = got[2]
                assert got[2][0]["waves_per_simd"] in ((1,) if name == "solve_w1" else (1, 2))
            results[(name, het is not None)] = got
    eng.clear_instance_consts()
    assert not eng.instance_consts_active()
    again = _step(eng, batch, "solve_w1")
    _same(again, results[("solve_w1", False)], f"{model} first solve again")
    assert eng.queue_info()[1:] == (B, 0)
    if model == "srbd13":                                       # the table mattered: another robot, another plan
        assert not np.array_equal(results[("solve_w1", True)][0][0], results[("solve_w1", False)][0][0])
    eng.close()
