"""Cost-to-go export on the device (include/sddp.h "cost-to-go export"): the value records out of the policy sweep against the numpy
recursion of tests/value_cases.py on every kernel family, the horizon edges, that the export changes nothing else, range and slot
independence, sddp_value_at_device against its stated arithmetic, the two experiments, refusals."""
import numpy as np
import pytest
import torch

from oracle import ddp as oddp, models as omodels
from srbd_horizon_amd import _lib, workload
from srbd_horizon_amd.engine import DdpEngine, eval_knots
from tests import failure_cases as fc, policy_cases as pc, value_cases as vc
from tests.gpu_support import solve as _solve
from tests.variant_cases import TRACKING, draw, extra_rows_problem

pytestmark = pytest.mark.gpu

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)      # dsrbd_example.py:55-58
EPS = np.finfo(float).eps


def _device_costs(model, N, x, u, P, consts):
    """L_k of one instance as the device's model code gives them (sddp_eval_knots), k = 0 .. N"""
    uu = np.concatenate([u, np.zeros((1, u.shape[1]))])
    return eval_knots(model, N, np.arange(N + 1), x, uu, P, consts)[4]


def _records(eng, nodes, first=0, count=None):
    eng.enable_value(nodes)
    eng.policy_range_device(first, count)
    return eng.fetch_value()


def _check_instance(model, N, b, rec, info, x, u, P, st, consts, rc, opt, nodes, label):
    """records [nodes, words] of instance b against oracle_values; c against the in-order sum of the device's own L"""
    m = omodels.make_model(model, rc)
    L = _device_costs(model, N, x, u, P, consts)
    ref = vc.oracle_values(m, x, u, P, st, opt, nodes, L=L)
    own = vc.oracle_values(m, x, u, P, st, opt, nodes)
    got = vc.split_records(rec, m.nx)
    print(f"{label}: max |c - c(oracle L)| / c = {np.max(np.abs(got['c'] - own['c']) / np.maximum(np.abs(own['c']), 1e-300)):.2e}, "
          f"max |Vxx - ref| / max |ref| = {np.max(np.abs(got['Vxx'] - ref['Vxx'])) / max(np.max(np.abs(ref['Vxx'])), 1e-300):.2e}")
    assert ref["ok"] == info[3] == 1.0, label
    vc.assert_values_match(got, ref, label)
    assert np.array_equal(got["Vxx"], np.swapaxes(got["Vxx"], -1, -2)), label
    assert got["expected"][0].tobytes() == info[2].tobytes(), label          # node 0: the bits of the policy record's word
    if nodes == N + 1:
        assert got["expected"][N] == 0.0


CASES = [("srbd13", 30, 16, 2, "plain"), ("srbd37", 20, 4, 2, "plain"), ("lip30", 20, 4, 2, "plain"), ("srbd61", 20, 3, 2, "plain"),
         ("srbd13", 30, 4, 2, "xr"), ("srbd13", 30, 4, 2, "tab"), ("srbd37", 20, 2, 1, "tab")]


@pytest.mark.parametrize("max_iters", [100, 3])
@pytest.mark.parametrize("model,N,B,slots,kind", CASES)
def test_value_records_match_the_numpy_recursion(model, N, B, slots, kind, max_iters):
    seeds = np.arange(B) + 3
    batch = workload.make_batch(model, N, seeds)
    P, consts = batch["params"], batch["consts"]
    if kind == "xr":
        batch, P, consts = extra_rows_problem(model, N, seeds)
    o = dict(OPTS, max_iters=max_iters)
    eng = DdpEngine(model, N, B, opts=dict(o, max_slots=slots), consts=consts)
    per = [(consts, omodels.RobotConsts(**consts))] * B
    if kind == "tab":
        over, csts = draw(batch["consts"], B, TRACKING, seed=3)
        eng.set_instance_consts(over)
        per = [(dict(consts, **{k: v[b] if np.ndim(v[b]) else float(v[b]) for k, v in over.items()}), csts[b]) for b in range(B)]
    eng.enable_policy(2)
    x, u, st = _solve(eng, batch, P)
    if max_iters == 3 and model == "srbd13":      # the one-wave sweep's open-gap (Vxx d) path is covered (the 4-wave sweep has one path:
        assert (st["gap"] > oddp.DdpOptions().gap_tol).any()      # closed gaps are zero defects there)
    opt = oddp.DdpOptions(**o)
    check = sorted(set(range(0, B, max(1, B // 4))) | {B - 1})
    for nodes in (1, 3, N + 1):
        rec = _records(eng, nodes)
        assert eng.value_words() == (nodes * vc.node_words(eng.nx), nodes) and rec.shape == (B, nodes, vc.node_words(eng.nx))
        assert eng.device_buffer(_lib.DEVICE_BUF_VALUE)[1] == rec.nbytes
        info = eng.policy()[2]
        for b in check if nodes == N + 1 else check[:2]:
            _check_instance(model, N, b, rec[b], info[b], x[b], u[b], P[b], st[b], per[b][0], per[b][1], opt, nodes,
                            f"{model} {kind} max_iters {max_iters} nodes {nodes} instance {b}")
    v = eng.value()
    assert v["c"].shape == (B, N + 1) and v["Vxx"].shape == (B, N + 1, eng.nx, eng.nx) and v["vx"].is_cuda
    np.testing.assert_array_equal(v["Vxx"].cpu().numpy(), vc.split_records(rec, eng.nx)["Vxx"])
    eng.close()


@pytest.mark.parametrize("model,N", [("srbd13", 1), ("srbd13", 2), ("srbd13", 64), ("srbd13", 65), ("srbd37", 1)])
def test_value_records_at_the_horizon_edges(model, N):
    """nodes = N + 1 where the knot loops' prefetch guards and the cost sum's 64-knot chunks change path"""
    B = 2
    batch = workload.make_batch(model, N, [0, 1])
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    eng.enable_policy(1)
    x, u, st = _solve(eng, batch)
    rec = _records(eng, N + 1)
    info = eng.policy()[2]
    for b in range(B):
        _check_instance(model, N, b, rec[b], info[b], x[b], u[b], batch["params"][b], st[b], batch["consts"],
                        omodels.RobotConsts(**batch["consts"]), oddp.DdpOptions(**OPTS), N + 1, f"{model} N = {N} instance {b}")
    eng.close()


@pytest.mark.parametrize("model,N,B", [("srbd13", 30, 8), ("srbd37", 20, 3)])
def test_the_export_changes_nothing_else(model, N, B):
    """solve results and policy records with the export on are the bytes of the same handle with it off, and so is a resumable
    handle's continue behind it"""
    batch = workload.make_batch(model, N, np.arange(B) + 5)

    def run(value):
        eng = DdpEngine(model, N, B, opts=dict(OPTS, max_iters=3, max_slots=3), consts=batch["consts"])
        eng.enable_resume()
        eng.enable_policy(4)
        if value:
            eng.enable_value(N + 1)
        out = list(_solve(eng, batch))
        eng.policy_range_device()
        out += [eng.fetch_policy(), *eng.fetch()]
        eng.set_options(max_iters=100)
        eng.continue_solve()
        out += list(eng.fetch())
        eng.policy_range_device()
        out += [eng.fetch_policy(), *eng.fetch()]
        if value:
            assert np.any(eng.fetch_value() != 0.0)
        eng.close()
        return out

    off, on = run(False), run(True)
    assert (off[2]["status"] == 1).any() and (off[9]["status"] == 0).all()
    for a, b in zip(off, on):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("model,N,B,slot_counts", [("srbd13", 30, 8, (3, 8)), ("srbd37", 20, 4, (1, 4))])
def test_records_and_value_at_are_bit_identical_across_ranges_and_slot_counts(model, N, B, slot_counts):
    batch = workload.make_batch(model, N, np.arange(B) + 11)
    nodes = 3
    xm = torch.from_numpy(batch["x0"] + 1e-2 * np.random.default_rng(1).standard_normal(batch["x0"].shape)).cuda()
    ref, at = None, {}
    for slots in slot_counts:
        eng = DdpEngine(model, N, B, opts=dict(OPTS, max_slots=slots), consts=batch["consts"])
        eng.enable_policy(1)
        _solve(eng, batch)
        whole = _records(eng, nodes).copy()
        assert np.all(eng.policy()[2][:, 3] == 1.0) and np.any(whole != 0.0)
        if ref is None:
            ref = whole
        assert whole.tobytes() == ref.tobytes()
        eng.enable_value(0); eng.enable_value(nodes)                       # a fresh (zeroed) buffer, filled by two halves
        eng.policy_range_device(0, B // 2); eng.policy_range_device(B // 2, B - B // 2)
        assert eng.fetch_value().tobytes() == ref.tobytes()
        eng.enable_value(0); eng.enable_value(nodes)
        for b in range(B):
            eng.policy_range_device(b, 1)
        assert eng.fetch_value().tobytes() == ref.tobytes()
        assert eng.fetch_value(1, 2).tobytes() == ref[1:3].tobytes()
        for node in (0, nodes - 1):
            def dev_at(first, count):                                     # device tensors in and out: asynchronous, so wait
                out = eng.value_at(xm[first:first + count].contiguous(), node, first, count)
                eng.synchronize()
                return out.cpu().numpy()
            w = dev_at(0, B)
            assert w.tobytes() == at.setdefault(node, w).tobytes()
            halves = np.concatenate([dev_at(0, B // 2), dev_at(B // 2, B - B // 2)])
            singles = np.concatenate([dev_at(b, 1) for b in range(B)])
            assert halves.tobytes() == w.tobytes() and singles.tobytes() == w.tobytes()
        eng.close()


@pytest.mark.parametrize("model,N,B", [("srbd13", 30, 4), ("srbd61", 20, 2)])
def test_value_at_against_the_stated_arithmetic(model, N, B):
    batch = workload.make_batch(model, N, np.arange(B) + 2)
    eng = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    eng.enable_policy(1)
    x, u, st = _solve(eng, batch)
    rec = vc.split_records(_records(eng, N + 1), eng.nx)
    rng = np.random.default_rng(7)
    for node in (0, N):
        w = eng.value_at(x[:, node].copy(), node=node)                       # delta = 0
        assert np.all(w[:, 1] == 0.0) and np.all(w[:, 2] == 0.0) and np.all(w[:, 5] == 0.0)
        np.testing.assert_array_equal(w[:, 0], rec["c"][:, node] + rec["expected"][:, node])
        np.testing.assert_array_equal(w[:, 3], rec["c"][:, node]); np.testing.assert_array_equal(w[:, 4], rec["expected"][:, node])
        assert np.all(w[:, 6] == 1.0) and np.all(w[:, 7] == node)
        xm = x[:, node] + 1e-2 * rng.standard_normal((B, eng.nx))
        w = eng.value_at(xm, node=node)
        for b in range(B):
            ref, mag = vc.value_at_reference(rec["c"][b, node], rec["expected"][b, node], rec["vx"][b, node], rec["Vxx"][b, node],
                                             xm[b] - x[b, node])
            err = np.abs(w[b, :3] - ref[:3])
            print(f"{model} node {node} instance {b}: |value, lin, quad - numpy| = {err}, 4 ulp of the terms = {4 * EPS * mag:.3e}")
            assert np.all(err <= 4 * EPS * mag)
            np.testing.assert_array_equal(w[b, 3:6], ref[3:6])
    eng.close()


def test_value_at_of_an_instance_without_a_policy_is_zeros():
    """a status-3 start (tests/failure_cases.py S3a: NaN in x0 and the warm start of some instances): ok = 0, every value word 0.0,
    words 0 .. 4 of sddp_value_at_device 0.0; the healthy instances beside them are untouched"""
    name = "S3a-srbd13"
    c, s = fc.CASES[name], fc.start(name)
    B = len(c.seeds)
    eng = DdpEngine("srbd13", c.N, B, consts=s["consts"])
    eng.enable_policy(1)
    x, u, st = _solve(eng, s)
    rec = _records(eng, 2)
    info = eng.policy()[2]
    w = eng.value_at(np.where(np.isfinite(s["x0"]), s["x0"], 0.0) + 1e-3, node=1)
    for b in range(B):
        if b in c.fail:
            assert st["status"][b] == 3 and info[b, 3] == 0.0
            assert np.all(rec[b] == 0.0) and np.all(w[b, :5] == 0.0) and w[b, 6] == 0.0 and w[b, 7] == 1.0
        else:
            assert info[b, 3] == 1.0 and w[b, 6] == 1.0 and w[b, 3] == rec[b, 1, 0] and w[b, 3] > 0.0 and np.isfinite(w[b]).all()
    eng.close()


@pytest.mark.parametrize("model", ["lip30", "srbd13"])
def test_experiments_on_the_device(model):
    """the cost of the converged re-solve from x0 + eps v against the value record of node 0 (tests/value_cases.py: lip30 exact within
    100 x the oracle's own error, srbd13 first-order decay); instances and eps chosen on the oracle (tests/test_value_cpu.py)"""
    N, seed = pc.FO_CASES[model]
    b = workload.make_batch(model, N, [seed, seed, seed])
    eng = DdpEngine(model, N, 3, opts=pc.FO_OPTS, consts=b["consts"])
    eng.enable_policy(1)
    x, u, st = _solve(eng, b)
    assert st["converged"].all()
    _records(eng, 1)
    v = pc.fo_direction(model, eng.nx)
    x0 = b["x0"].copy()
    x0[1] += pc.FO_EPS[0] * v
    x0[2] += pc.FO_EPS[1] * v
    w = eng.value_at(x0, node=0)
    assert np.all(w[:, 6] == 1.0)
    eng.load(x0, x, u)
    eng.solve(b["params"])
    assert eng.stats["converged"].all()
    J = eng.stats["cost"].copy()
    print(f"{model}: c_0 = {w[0, 3]:.6e}, expected_0 = {w[0, 4]:.3e}, lin = {w[1:, 1]}, quad = {w[1:, 2]}, J* = {J[1:]}")
    vc.assert_experiment(model, vc.value_errors(model, w[0, 3], w[0, 4], w[1:, 1], w[1:, 2], J[1:]))
    eng.close()


def test_value_refusals():
    batch = workload.make_batch("srbd13", 30, [0, 1])
    eng = DdpEngine("srbd13", 30, 2, opts=OPTS)
    xm = torch.zeros((2, 13), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="sddp_enable_policy first"):                # before enable_policy
        eng.enable_value(1)
    for call in (eng.value_words, eng.fetch_value, lambda: eng.value_at(xm), lambda: eng.device_buffer(_lib.DEVICE_BUF_VALUE)):
        with pytest.raises(RuntimeError, match="sddp_enable_value"):
            call()
    eng.enable_policy(2)
    for nodes in (-1, 32):
        with pytest.raises(RuntimeError, match=r"nodes must be in 1\.\.N\+1"):
            eng.enable_value(nodes)
    eng.enable_value(31)
    assert eng.value_words() == (31 * 184, 31)
    eng.enable_value(3)
    with pytest.raises(RuntimeError, match="no solve has run"):
        eng.value_at(xm)
    _solve(eng, batch)
    eng.policy_range_device()
    assert eng.value_at(xm, node=2).shape == (2, 8)
    for node in (-1, 3):
        with pytest.raises(RuntimeError, match="kept node"):
            eng.value_at(xm, node=node)
    with pytest.raises(RuntimeError, match="range outside"):
        eng.value_at(xm, node=0, first=1, count=2)
    eng.enable_policy(0)                                                               # drops the export with the policy
    with pytest.raises(RuntimeError, match="sddp_enable_value"):
        eng.fetch_value()
    eng.close()
    so2 = DdpEngine("srbd13", 30, 2, opts=dict(OPTS, second_order=2))
    bar = DdpEngine("srbd37", 20, 1, opts=OPTS, consts=dict(friction_barrier_weight=1e-3, friction_barrier_sharpness=5.0))
    for e in (so2, bar):                                                               # no policy exists there, so no value export
        with pytest.raises(RuntimeError, match="sddp_enable_policy first"):
            e.enable_value(1)
        e.close()
