"""Policy export on the device (include/sddp.h "policy export"): the gains of the first M knots of every instance, from ONE backward
sweep at the RETURNED iterate, against the numpy oracle evaluated by the rule that tests/policy_cases.py states; queue independence;
the mode-2 gather record; sddp_apply_policy_device; the first-order property of the gains; MpcLoop with feedback; refusals."""
import os

import numpy as np
import pytest
import torch

from oracle import cport, ddp as oddp, models as omodels
from srbd_horizon_amd import dist as sdist, workload
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.mpc import MpcLoop
from tests import policy_cases as pc
from tests.gpu_support import solve as _solve
from tests.variant_cases import extra_rows_problem

pytestmark = pytest.mark.gpu

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)      # dsrbd_example.py:55-58
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _x_problem(model, N, seeds):
    """the "_x" build's problem of tests/test_gpu_extra_rows.py: four linear user rows, two with per-knot references"""
    return extra_rows_problem(model, N, seeds)


@pytest.mark.parametrize("model,N,B,slots,xr,max_iters", [
    ("srbd13", 30, 192, 40, False, 100), ("srbd13", 30, 192, 40, False, 3), ("srbd37", 20, 6, 2, False, 100),
    ("srbd37", 20, 6, 2, False, 3), ("lip30", 20, 6, 4, False, 100), ("srbd61", 20, 3, 2, False, 100), ("srbd13", 30, 12, 5, True, 100)])
def test_policy_matches_the_oracle_sweep_at_the_returned_iterate(model, N, B, slots, xr, max_iters):
    M = 4
    seeds = np.arange(B) + 3
    if xr:
        batch, P, consts = _x_problem(model, N, seeds)
    else:
        batch = workload.make_batch(model, N, seeds)
        P, consts = batch["params"], batch["consts"]
    o = dict(OPTS, max_iters=max_iters)
    eng = DdpEngine(model, N, B, opts=dict(o, max_slots=slots), consts=consts)
    eng.enable_policy(M)
    nx, nu = eng.nx, eng.nu
    assert eng.policy_words() == (M * nu * (nx + 1) + 4, M)
    x, u, st = _solve(eng, batch, P)
    assert eng.queue_info()[1:] == (slots, B)                          # the solve was a queue: no gains from sddp_device_ptr(3)
    with pytest.raises(RuntimeError, match="per queue slot"):
        eng.device_buffer(3)
    eng.policy_range_device()
    kff, K, info = eng.policy()
    assert kff.shape == (B, M, nu) and K.shape == (B, M, nu, nx) and info.shape == (B, 4)
    x2, u2, st2 = eng.fetch()                                          # the policy launch changes no result of the solve
    np.testing.assert_array_equal(x2, x); np.testing.assert_array_equal(u2, u)
    for f in st.dtype.names:
        np.testing.assert_array_equal(st2[f], st[f], err_msg=f)
    m = omodels.make_model(model, omodels.RobotConsts(**consts))
    opt = oddp.DdpOptions(**o)
    if max_iters == 3:
        assert (st["status"] == 1).any()                               # instances that end by max_iters are covered
    check = sorted(set(range(0, B, max(1, B // 24))) | set(np.flatnonzero(st["status"] != 0)[:8].tolist()))
    for b in check:
        ref = pc.oracle_policy(m, x[b], u[b], P[b], st[b], opt, M)
        pc.assert_policy_matches(kff[b], K[b], info[b], ref, label=f"{model} instance {b} status {st['status'][b]}")
    assert (info[:, 3] == 1.0).all()


@pytest.mark.parametrize("model,N,B", [("srbd13", 30, 16), ("srbd37", 20, 4)])
def test_policy_differs_from_the_slot_gains_after_max_iters(model, N, B):
    """The case that makes the export necessary: a solve that ends by max_iters ran its last sweep at the PREVIOUS iterate, so the
    gains in the slots' work buffer (sddp_device_ptr(3), readable here: no queue) are not those of the returned trajectory; the
    exported ones are (oracle sweep at the returned iterate)."""
    M = 4
    batch = workload.make_batch(model, N, np.arange(B) + 3)
    o = dict(OPTS, max_iters=3)
    eng = DdpEngine(model, N, B, opts=o, consts=batch["consts"])
    eng.enable_policy(M)
    x, u, st = _solve(eng, batch)
    eng.policy_range_device()
    kff, K, info = eng.policy()
    g = eng.device_view(3, (B, N, eng.nu * (eng.nx + 1))).cpu().numpy().copy()
    K3 = g[:, :M, eng.nu:].reshape(B, M, eng.nu, eng.nx)
    m = omodels.make_model(model, omodels.RobotConsts(**batch["consts"]))
    cut = np.flatnonzero((st["status"] == 1) & (st["iters"] == 3))
    assert len(cut) >= 2
    for b in cut:
        pc.assert_policy_matches(kff[b], K[b], info[b], pc.oracle_policy(m, x[b], u[b], batch["params"][b], st[b], oddp.DdpOptions(**o), M),
                                 label=f"instance {b}")
        diff = np.max(np.abs(K3[b] - K[b])) / np.max(np.abs(K[b]))
        print(f"{model} instance {b}: max |K(which = 3) - K(policy)| / max |K| = {diff:.3e}")
        assert diff > 1e-6


def test_policy_is_bit_identical_across_ranges_and_slot_counts():
    model, N, B, M = "srbd13", 30, 64, 2
    batch = workload.make_batch(model, N, np.arange(B) + 11)
    ref = DdpEngine(model, N, B, opts=OPTS)
    ref.enable_policy(M)
    _solve(ref, batch)
    ref.policy_range_device()
    r0 = ref.fetch_policy()
    assert np.all(r0[:, -1] == 1.0)
    for slots in (7, 33):
        q = DdpEngine(model, N, B, opts=dict(OPTS, max_slots=slots))
        q.enable_policy(M)
        _solve(q, batch)
        q.policy_range_device(0, 20)
        q.policy_range_device(20, 44)
        np.testing.assert_array_equal(q.fetch_policy(), r0)
        q.policy_range_device(5, 3)                                    # again, a short range without a queue
        np.testing.assert_array_equal(q.fetch_policy(), r0)
        np.testing.assert_array_equal(q.fetch_policy(5, 3), r0[5:8])
    m4 = DdpEngine("srbd37", 20, 5, opts=OPTS)
    m4q = DdpEngine("srbd37", 20, 5, opts=dict(OPTS, max_slots=2))
    b4 = workload.make_batch("srbd37", 20, np.arange(5) + 1)
    out = []
    for e in (m4, m4q):
        e.enable_policy(M)
        _solve(e, b4)
        e.policy_range_device()
        out.append(e.fetch_policy())
    np.testing.assert_array_equal(out[0], out[1])


def test_mode2_records_are_mode1_records_plus_the_first_knots_gains():
    model, N, B = "srbd13", 30, 48
    dev = torch.device("cuda", 0)
    batch = workload.make_batch(model, N, np.arange(B) + 2)
    eng = DdpEngine(model, N, B, opts=dict(OPTS, max_slots=16))
    eng.enable_policy(3)
    x, u, st = _solve(eng, batch)
    eng.policy_range_device()
    pol = eng.fetch_policy()
    nu, nx = eng.nu, eng.nx
    W1, W2 = eng.record_words("first_knot"), eng.record_words("first_knot_policy")
    assert W2 == W1 + nu * (nx + 1) == sdist.record_words(N, nx, nu, "first_knot_policy")
    for first, count in ((0, B), (7, 30)):
        r1 = eng.pack_records_device(torch.empty((count, W1), dtype=torch.float64, device=dev), first, count, "first_knot")
        r2 = eng.pack_records_device(torch.empty((count, W2), dtype=torch.float64, device=dev), first, count, "first_knot_policy")
        r0 = eng.pack_records_device(torch.empty((count, eng.record_words("full")), dtype=torch.float64, device=dev), first, count, "full")
        eng.synchronize()
        r0, r1, r2 = r0.cpu().numpy(), r1.cpu().numpy(), r2.cpu().numpy()
        sl = slice(first, first + count)
        np.testing.assert_array_equal(r2[:, :W1], r1)
        np.testing.assert_array_equal(r2[:, W1:], pol[sl, :nu * (nx + 1)])
        for mode, got in (("full", r0), ("first_knot", r1)):          # modes 0 and 1 as before: the host-side packing
            ref = torch.empty(got.shape, dtype=torch.float64)
            sdist.pack_records_into(ref, torch.from_numpy(x[sl]), torch.from_numpy(u[sl]), torch.from_numpy(st["cost"][sl].copy()),
                                    torch.from_numpy(st["iters"][sl].copy()), mode)
            np.testing.assert_array_equal(got, ref.numpy())


@pytest.mark.parametrize("model,N,B", [("srbd13", 30, 40), ("srbd61", 20, 3)])
def test_apply_policy_device(model, N, B):
    dev = torch.device("cuda", 0)
    batch = workload.make_batch(model, N, np.arange(B) + 5)
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    eng.enable_policy(1)
    x, u, st = _solve(eng, batch)
    eng.policy_range_device()
    _, K, _ = eng.policy()
    rng = np.random.default_rng(3)
    for first, count in ((0, B), (1, B - 2)):
        dx = 1e-2 * rng.standard_normal((count, eng.nx))
        xm = x[first:first + count, 0] + dx
        out = torch.empty((count, eng.nu), dtype=torch.float64, device=dev)
        eng.apply_policy_device(torch.from_numpy(xm).to(dev), out, first, count)
        eng.synchronize()
        got = out.cpu().numpy()
        K0 = K[first:first + count, 0]
        ref = u[first:first + count, 0] + np.einsum("bij,bj->bi", K0, xm - x[first:first + count, 0])
        scale = np.max(np.abs(K0)) * np.max(np.abs(xm - x[first:first + count, 0])) * eng.nx
        err = np.max(np.abs(got - ref))
        print(f"{model} apply_policy: max error {err:.3e}, bound {1e-12 * scale:.3e}")
        assert err <= 1e-12 * scale


@pytest.mark.parametrize("model", ["lip30", "srbd13"])
def test_first_order_property_of_the_exported_gains(model):
    """u_0 of the problem re-solved from x0 + eps v against the policy's prediction u_0 + K_0 eps v: the error falls like eps^2
    (tests/policy_cases.py assert_first_order; instances and eps chosen on the oracle, tests/test_policy_cpu.py)."""
    N, seed = pc.FO_CASES[model]
    b = workload.make_batch(model, N, [seed, seed, seed])
    eng = DdpEngine(model, N, 3, opts=pc.FO_OPTS, consts=b["consts"])
    eng.enable_policy(1)
    x, u, st = _solve(eng, b)
    assert st["converged"].all()
    eng.policy_range_device()
    _, K, info = eng.policy()
    assert info[0, 3] == 1.0
    v = pc.fo_direction(model, eng.nx)
    x0 = b["x0"].copy()
    x0[1] += pc.FO_EPS[0] * v
    x0[2] += pc.FO_EPS[1] * v
    eng.load(x0, x, u)
    x2, u2 = eng.solve(b["params"])
    assert eng.stats["converged"].all()
    pc.assert_first_order(model, pc.fo_errors(u[0, 0], K[0, 0], v, lambda eps: u2[1 + pc.FO_EPS.index(eps), 0]))


def test_mpc_loop_default_reproduces_the_recorded_ticks_and_feedback_rejects_a_push():
    """feedback_substeps = 0: the srbd37 walking loop's 20 ticks, bit for bit the record taken before MpcLoop knew of the policy
    (tests/golden/mpc_srbd37_ticks20.npz).  feedback_substeps = 4 with a lateral push (2 m/s^2 on the CoM over ticks 6..9): the
    peak lateral CoM deviation from the unpushed run is smaller with the policy than with the first input applied open loop over
    the same sub-steps (direction only; the two numbers are printed)."""
    g = np.load(os.path.join(GOLDEN, "mpc_srbd37_ticks20.npz"))
    lp = MpcLoop("srbd37", 20, feedback_substeps=0)
    states, u0s = [lp.state.copy()], []
    for _ in range(20):
        _, sol = lp.tick("walking", (1.0, 0.0))
        states.append(lp.state.copy()); u0s.append(sol["u_opt"][:, 0].copy())
    np.testing.assert_array_equal(np.array(states), g["states"])
    np.testing.assert_array_equal(np.array(u0s), g["u0"])

    def run(feedback, push):
        lp = MpcLoop("srbd37", 20, feedback_substeps=4, feedback=feedback)
        y = []
        for t in range(20):
            lp.tick("walking", (1.0, 0.0), push=(0.0, 2.0, 0.0) if (push and 6 <= t <= 9) else None)
            y.append(lp.state[1])
        return np.array(y)

    dev_open = np.max(np.abs(run(False, True) - run(False, False)))
    dev_pol = np.max(np.abs(run(True, True) - run(True, False)))
    print(f"peak lateral CoM deviation after the push: open loop {dev_open:.5f} m, with the policy {dev_pol:.5f} m")
    assert dev_pol < dev_open


def test_policy_refusals():
    batch = workload.make_batch("srbd13", 30, [0, 1])
    eng = DdpEngine("srbd13", 30, 2, opts=OPTS)
    for call in (eng.policy_words, eng.policy_range_device, eng.fetch_policy, lambda: eng.device_buffer(8),
                 lambda: eng.record_words("first_knot_policy")):
        with pytest.raises(RuntimeError, match="sddp_enable_policy"):                 # nothing enabled
            call()
    for knots in (-1, 31):
        with pytest.raises(RuntimeError, match="knots must be in 1..N"):
            eng.enable_policy(knots)
    eng.enable_policy(30)
    assert eng.policy_words() == (30 * 6 * 14 + 4, 30)
    assert eng.device_buffer(8)[1] == 2 * (30 * 6 * 14 + 4) * 8
    with pytest.raises(RuntimeError, match="no solve has run"):                       # policy before any solve
        eng.policy_range_device()
    _solve(eng, batch)
    with pytest.raises(RuntimeError, match="range outside"):
        eng.policy_range_device(1, 2)
    eng.policy_range_device()
    assert eng.fetch_policy().shape == (2, 30 * 6 * 14 + 4)
    eng.enable_policy(0)                                                              # frees it
    with pytest.raises(RuntimeError, match="sddp_enable_policy"):
        eng.fetch_policy()
    with pytest.raises(RuntimeError, match="sddp_enable_policy"):
        eng.pack_records_device(torch.empty((2, 21), dtype=torch.float64, device="cuda"), 0, 2, "first_knot_policy")
    so2 = DdpEngine("srbd13", 30, 2, opts=dict(OPTS, second_order=2))
    with pytest.raises(RuntimeError, match="no policy kernel"):
        so2.enable_policy(1)
    bar = DdpEngine("srbd37", 20, 1, opts=OPTS, consts=dict(friction_barrier_weight=1e-3, friction_barrier_sharpness=5.0))
    with pytest.raises(RuntimeError, match="no policy kernel"):
        bar.enable_policy(1)
