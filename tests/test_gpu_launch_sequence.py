"""One solve launch is a sequence on the handle's stream: deadline stamp, class labels, queue-order pre-pass,
solve kernel, class update, timing events around all of it.  Two of its paths that no other test walks:

1. a USER build (tests/user_terms_defs.py, loaded from a shared object of its own) behind a queue under every queue order: results
   bit-exact against the same batch on one workgroup per instance;
2. the timing events bracket a whole sequence, once per launch, whatever the pre-pass in front of the solve kernel is.
"""
import numpy as np
import pytest
import torch

from srbd_horizon_amd import workload
from srbd_horizon_amd.engine import DdpEngine
from tests.user_terms_defs import user_case as _user_case, widen as _widen

pytestmark = pytest.mark.gpu

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
# (case of tests/user_terms_defs.all_specs, model, its N, instances, max_slots, waves_per_simd): the one-wave and the four-wave kernel
USER_CASES = {"one_wave": ("srbd13_terrain", "srbd13", 20, 24, 4, 2), "four_wave": ("srbd37_reach", "srbd37", 20, 6, 2, 1)}
N_CLASSES = 3


def _solve(eng, batch, P):
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(P)
    return x.copy(), u.copy(), eng.stats.tobytes()


@pytest.fixture(scope="module", params=sorted(USER_CASES))
def user_case(request):
    """The user build, its batch and the reference: the batch on a handle without max_slots (one workgroup per instance, no queue)."""
    case, model, N, B, slots, wps = USER_CASES[request.param]
    spec, mid = _user_case(case, N)
    batch = workload.make_batch(model, N, np.arange(B) + 5)
    P = _widen(batch["params"], spec, vary=0.1)
    consts = dict(batch["consts"], extra_rows=spec.extra_rows())
    ref = DdpEngine(model, N, B, opts=dict(OPTS, waves_per_simd=wps), consts=consts, model_id=mid)
    want = _solve(ref, batch, P)
    assert ref.queue_info() == (B, B, 0)
    ref.close()
    return dict(model=model, N=N, B=B, slots=slots, wps=wps, mid=mid, batch=batch, P=P, consts=consts, want=want)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_user_build_behind_a_queue(user_case, order):
    c = user_case
    B, slots = c["B"], c["slots"]
    x0, u0, s0 = c["want"]
    eng = DdpEngine(c["model"], c["N"], B, opts=dict(OPTS, max_slots=slots, waves_per_simd=c["wps"], queue_order=order), consts=c["consts"],
                    model_id=c["mid"])
    assert eng.queue_info()[0] == slots
    labels = (np.arange(B) % N_CLASSES).astype(np.int32)
    if order == 3:
        eng.set_instance_classes(labels, N_CLASSES)
    launches = 2 if order in (1, 3) else 1      # order 1: the second launch has `hist`; order 3: ... a class history
    for launch in range(launches):
        x, u, s = _solve(eng, c["batch"], c["P"])
        np.testing.assert_array_equal(x, x0)
        np.testing.assert_array_equal(u, u0)
        assert s == s0, f"sddp_stats bytes of launch {launch}"
        assert eng.queue_info() == (slots, slots, B)
        if order >= 1:
            assert sorted(eng.last_queue_order().tolist()) == list(range(B))
    if order == 3:
        for cls in range(N_CLASSES):
            assert eng.class_history(cls)[1] == launches * int((labels == cls).sum())
    eng.close()


def _timed_engine(B=24, N=10, **over):
    batch = workload.make_batch("srbd13", N, np.arange(B) + 5)
    eng = DdpEngine("srbd13", N, B, opts=dict(OPTS, max_slots=4, **over))
    eng.use_torch_stream(torch.cuda.current_stream())
    dev = {k: torch.tensor(batch[k], dtype=torch.float64, device="cuda") for k in ("x0", "xs", "us", "params")}
    eng.set_initial_state_device(dev["x0"]); eng.set_x_warmstart_device(dev["xs"]); eng.set_u_warmstart_device(dev["us"])
    return eng, dev


@pytest.mark.parametrize("order", [0, 2, 3])
def test_timing_brackets_every_launch_once(order):
    eng, dev = _timed_engine(queue_order=order)
    if order == 3:
        eng.enable_auto_classes()
    eng.enable_timing()
    _, n0 = eng.kernel_time_stats()
    for _ in range(3):
        eng.solve_device(dev["params"])
    eng.synchronize()
    total, n = eng.kernel_time_stats()
    print(f"queue_order {order}: {n - n0} intervals, sum {total:.3f} ms, last {eng.last_kernel_ms():.3f} ms")
    assert eng.queue_info()[1:] == (4, 24)
    assert n - n0 == 3 and total > 0.0 and eng.last_kernel_ms() > 0.0
    eng.close()


def test_timing_brackets_a_continue_launch_once():
    eng, dev = _timed_engine(max_iters=2)
    eng.enable_resume()
    eng.solve_device(dev["params"])                     # cut at max_iters = 2
    assert eng.unfinished() > 0
    eng.set_options(max_iters=100)
    eng.enable_timing()
    _, n0 = eng.kernel_time_stats()
    eng.continue_solve(dev["params"])
    eng.synchronize()
    total, n = eng.kernel_time_stats()
    print(f"continue launch: {n - n0} intervals, sum {total:.3f} ms, last {eng.last_kernel_ms():.3f} ms")
    assert n - n0 == 1 and total > 0.0 and eng.last_kernel_ms() > 0.0
    eng.close()
