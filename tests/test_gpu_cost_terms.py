"""Cost breakdown on the device (include/sddp.h sddp_cost_terms_range_device, sddp_cost_terms): the record and the per-node addends of
every kernel family and build kind against statement A of tests/cost_terms_cases.py (the oracle's cost with the gains masked family
by family) on the device's own fetched x, u, P, and what the record promises exactly.

Tolerance (cost_terms_cases.tolerances): per family, 64 x the A-versus-B disagreement of the two CPU statements committed in
profiles/cost_terms/cpu_disagreement.json, relative to the record's word; a family on which the two CPU statements agree to less than
one rounding (they share the rows' values sqrt(w) e and differ in the order of one sum only) is given 64 x eps, since the device forms
w e^2 where both of them form (sqrt(w) e)^2.  Every test prints its worst |difference| / tolerance.
"""
import ctypes as C
import dataclasses
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import models as omodels
from srbd_horizon_amd import _lib, workload
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.fleet import FleetQueue
from tests import cost_terms_cases as cc
from tests.gpu_support import BUILDS, solve
from tests.variant_cases import SRBD13_FIELDS, draw

pytestmark = pytest.mark.gpu

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
B = 6
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cost_terms", "cpu_disagreement.json")) as _f:
    TOL = cc.tolerances(json.load(_f))
FAM = slice(1, 1 + cc.FAMILIES)


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda")


def _run(eng, first=0, count=None, x=None, u=None, nodes=True):
    """cost_terms_device on fresh device tensors -> numpy (record [n, 16], addends [n, N + 1, 14] or None)"""
    n = eng.B - first if count is None else count
    out = torch.full((n, cc.WORDS), 7.0, dtype=torch.float64, device="cuda")
    nd = torch.full((n, eng.N + 1, cc.COLS), 7.0, dtype=torch.float64, device="cuda") if nodes else None
    eng.cost_terms_device(out, first, n, x=None if x is None else _dev(x), u=None if u is None else _dev(u), nodes=nd)
    eng.synchronize()
    return out.cpu().numpy(), (nd.cpu().numpy() if nodes else None)


def _problem(model, N, kind, nb=B):
    """-> (batch, P, consts dict, opts) of a case: seeds 3 .. of srbd_horizon_amd.workload"""
    batch = workload.make_batch(model, N, np.arange(nb) + 3)
    P = batch["params"]
    consts = dict(batch["consts"], **cc.consts_of(model, kind))
    if kind == "x":
        P = np.concatenate([P, np.zeros((nb, N + 1, 8))], axis=2)
        P[:, :, P.shape[2] - 8] = 0.02 * np.sin(np.arange(N + 1) / 5.0)[None]
        P[:, :, P.shape[2] - 6] = 0.1 * np.cos(np.arange(N + 1) / 3.0)[None]
    return batch, P, consts, dict(OPTS, **(dict(second_order=2) if kind == "so2" else {}))


@functools.lru_cache(maxsize=None)
def _solved(model, N, wps=1, kind="plain", nb=B):
    """a handle with its solve done, and what it gave: computed once, arrays read-only"""
    batch, P, consts, opts = _problem(model, N, kind, nb)
    eng = DdpEngine(model, N, nb, opts=dict(opts, waves_per_simd=wps), consts=consts)
    x, u, st = solve(eng, batch, P)
    for a in (x, u, st, P):
        a.setflags(write=False)
    return eng, omodels.RobotConsts(**consts), batch, x, u, st, P


def _random_plan(batch, seed=11):
    rng = np.random.default_rng(seed)
    return batch["xs"] + 0.03 * rng.standard_normal(batch["xs"].shape), batch["us"] + 0.03 * rng.standard_normal(batch["us"].shape)


def _check(model, cst, got, x, u, P, label, cols=range(cc.COLS)):
    rec, nodes = got
    worst = 0.0
    tol = np.array([TOL[c] if c in cols else np.inf for c in range(cc.COLS)])
    for b in range(rec.shape[0]):
        c = cst[b] if isinstance(cst, (list, tuple)) else cst
        worst = max(worst, cc.assert_against(rec[b], None if nodes is None else nodes[b], cc.statement_a(model, c, x[b], u[b], P[b]), tol,
                                             label=f"{label} instance {b}"))
    print(f"{label}: worst |difference| / tolerance {worst:.3f}")
    return worst


def _exact(rec, nodes):
    """what a record promises of itself, without a tolerance"""
    for b in range(rec.shape[0]):
        assert rec[b].tobytes() == cc.record_of(nodes[b]).tobytes(), b              # the in-order sum of its own rows; words 14, 15
        fam = rec[b, FAM]
        assert abs(fam.sum() - rec[b, cc.TOTAL]) <= 14 * cc.EPS * np.abs(fam).sum(), b


CASES = [(m, N, w) for m, ws in BUILDS.items() for N in (3, 5) for w in ws] + [("srbd13", 30, 1)]


@pytest.mark.parametrize("model,N,wps", CASES)
def test_every_model_against_statement_a(model, N, wps):
    eng, cst, batch, x, u, st, P = _solved(model, N, wps)
    own = _run(eng)
    _check(model, cst, own, x, u, P, f"{model} N = {N} wps = {wps} plan")
    _exact(*own)
    miss = np.max(np.abs(own[0][:, cc.TOTAL] - st["cost"]) / np.abs(st["cost"]))
    print(f"{model} N = {N}: word 0 against stats.cost (another order of the sum), largest relative difference {miss:.3e}; status {st['status']}")
    same = _run(eng, x=x, u=u)                                                      # d_x = NULL is the caller path fed the fetched plan
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(same, own))
    rx, ru = _random_plan(batch)
    rand = _run(eng, x=rx, u=ru)
    _check(model, cst, rand, rx, ru, P, f"{model} N = {N} wps = {wps} random trajectory")
    _exact(*rand)
    assert _run(eng, nodes=False)[0].tobytes() == own[0].tobytes()                  # d_nodes NULL
    for first, count in ((1, 3), (4, 1)):                                           # alone, in a sub-range, in the whole batch
        part = _run(eng, first, count)
        assert all(a.tobytes() == b_[first:first + count].tobytes() for a, b_ in zip(part, own)), (first, count)
        part = _run(eng, first, count, x=rx[first:first + count], u=ru[first:first + count])
        assert all(a.tobytes() == b_[first:first + count].tobytes() for a, b_ in zip(part, rand)), (first, count)
    host = eng.cost_terms(nodes=True)
    assert host["record"].tobytes() == own[0].tobytes() and host["nodes"].tobytes() == own[1].tobytes()
    assert host["total"].tobytes() == own[0][:, 0].tobytes() and list(host["largest"]) == [cc.NAMES[int(i)] for i in own[0][:, cc.LARGEST]]
    assert all(host[name].tobytes() == own[0][:, 1 + f].tobytes() for f, name in enumerate(cc.NAMES))
    assert eng.cost_terms(1, 2)["record"].tobytes() == own[0][1:3].tobytes()


def _records_with(model, N, consts, batch, rx, ru):
    eng = DdpEngine(model, N, rx.shape[0], opts=dict(OPTS, max_iters=0), consts=consts)
    solve(eng, batch)
    rec, _ = _run(eng, x=rx, u=ru)
    eng.close()
    return rec


@pytest.mark.parametrize("model,gains", [("srbd37", cc.GAINS[:7]), ("lip30", (cc.GAINS[7],))])
def test_a_gain_times_two_doubles_its_family_and_zero_removes_it(model, gains):
    N, nb = 3, 2
    batch = workload.make_batch(model, N, np.arange(nb) + 3)
    rx, ru = _random_plan(batch)
    ref = _records_with(model, N, batch["consts"], batch, rx, ru)
    for gain in gains:
        f = cc.GAINS.index(gain)
        value = getattr(omodels.RobotConsts(**batch["consts"]), gain)
        assert np.all(ref[:, 1 + f] > 0.0), gain
        others = [c for c in range(1, 1 + cc.FAMILIES) if c != 1 + f]
        twice = _records_with(model, N, dict(batch["consts"], **{gain: 2.0 * value}), batch, rx, ru)
        assert twice[:, 1 + f].tobytes() == (2.0 * ref[:, 1 + f]).tobytes(), gain
        assert twice[:, others].tobytes() == ref[:, others].tobytes(), gain
        none = _records_with(model, N, dict(batch["consts"], **{gain: 0.0}), batch, rx, ru)
        assert np.all(none[:, 1 + f] == 0.0) and none[:, others].tobytes() == ref[:, others].tobytes(), gain


def test_the_x_build_and_its_user_rows():
    model, N = "srbd13", 5
    eng, cst, batch, x, u, st, P = _solved(model, N, 1, "x")
    assert isinstance(omodels.make_model(model, cst), omodels.WithLinearRows) and len(cst.extra_rows) == 3
    rx, ru = _random_plan(batch)
    got = _run(eng, x=rx, u=ru)
    _check(model, cst, got, rx, ru, P, "srbd13_x random trajectory")
    _exact(*got)
    assert np.all(got[0][:, 1 + 11] > 0.0)
    own = _run(eng)
    _check(model, cst, own, x, u, P, "srbd13_x plan")
    # every other family: the bits of a plain handle fed the same trajectory
    plain = _solved(model, N, 1)[0]
    ref = _run(plain, x=rx, u=ru)
    others = [c for c in range(1, 1 + cc.FAMILIES) if c != 1 + 11]
    assert got[0][:, others].tobytes() == ref[0][:, others].tobytes() and got[1][:, :, others].tobytes() == ref[1][:, :, others].tobytes()
    assert np.all(ref[0][:, 1 + 11] == 0.0)


@pytest.mark.parametrize("kind,family", [("bar", 9), ("box", 10)])
def test_the_barrier_builds(kind, family):
    model, N = "srbd13", 5
    eng, cst, batch, x, u, st, P = _solved(model, N, 1, kind)
    own = _run(eng)
    _check(model, cst, own, x, u, P, f"srbd13 {kind} plan")
    _exact(*own)
    rx, ru = _random_plan(batch)
    _check(model, cst, _run(eng, x=rx, u=ru), rx, ru, P, f"srbd13 {kind} random trajectory")
    assert np.all(own[0][:, 1 + family] > 0.0) and np.all(own[0][:, 1 + (19 - family)] == 0.0)      # the one barrier, not the other


def test_the_second_order_build():
    model, N = "srbd13", 5
    eng, cst, batch, x, u, st, P = _solved(model, N, 1, "so2")
    own = _run(eng)
    _check(model, cst, own, x, u, P, "srbd13 so2 plan")
    _exact(*own)


def test_a_user_build():
    pytest.importorskip("sympy", reason="user builds are generated with sympy")
    from tests import user_terms_defs as defs
    model, N, nb = "srbd13", 20, 2
    spec, mid = defs.user_case("srbd13_pair", N)
    batch = workload.make_batch(model, N, np.arange(nb) + 3)
    P = defs.widen(batch["params"], spec)
    a0 = np.zeros(19); a0[7] = 1.0; a0[0] = 0.2                                   # the same two rows as linear rows of the _x build
    a1 = np.zeros(19); a1[13 + 2] = 1.0; a1[13 + 5] = -1.0
    lin = [dict(a=a0, w=defs.PAIR_GAINS[0], kind="state"), dict(a=a1, w=defs.PAIR_GAINS[1], kind="stage")]
    rx, ru = _random_plan(batch)
    recs = []
    for consts, m in ((dict(batch["consts"], extra_rows=spec.extra_rows()), mid), (dict(batch["consts"], extra_rows=lin), None)):
        eng = DdpEngine(model, N, nb, opts=dict(OPTS, max_iters=0), consts=consts, model_id=m)
        solve(eng, batch, P)
        recs.append(_run(eng, x=rx, u=ru))
        eng.close()
    (ur, un), (xr, xn) = recs
    _exact(ur, un)
    others = [c for c in range(1, 1 + cc.FAMILIES) if c != 1 + 11]
    assert ur[:, others].tobytes() == xr[:, others].tobytes() and un[:, :, others].tobytes() == xn[:, :, others].tobytes()
    # family 11 of a user build is a difference of two node costs (include/sddp.h): within the tolerance of user_rows and of what was
    # subtracted, of the linear rows' value, which test_the_x_build_and_its_user_rows holds against the oracle
    bound = TOL[12] * np.abs(xr[:, 12]) + TOL[13] * np.abs(xr[:, 13])
    print(f"user build: family 11 {ur[:, 12]}, linear rows {xr[:, 12]}, |difference| / bound {np.abs(ur[:, 12] - xr[:, 12]) / bound}")
    assert np.all(xr[:, 12] > 0.0) and np.all(np.abs(ur[:, 12] - xr[:, 12]) <= bound)


def test_instance_constants():
    model, N = "srbd13", 5
    eng, cst, batch, x, u, st, P = _solved(model, N, 1)
    rx, ru = _random_plan(batch)
    ref = _run(eng, x=rx, u=ru)
    tab = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])                 # a table equal to the handle's consts: the same bytes
    tab.set_instance_consts(dict(m=np.full(B, tab.consts.m)))
    assert tab.instance_consts_active()
    solve(tab, batch)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(_run(tab, x=rx, u=ru), ref))
    tab.close()
    over, csts = draw(batch["consts"], B, SRBD13_FIELDS, seed=3)                    # every robot its own gains, mass and inertia
    het = DdpEngine(model, N, B, opts=OPTS, consts=batch["consts"])
    het.set_instance_consts(over)
    xh, uh, _ = solve(het, batch)
    _check(model, csts, _run(het), xh, uh, P, "heterogeneous fleet plan")
    got = _run(het, x=rx, u=ru)
    _check(model, csts, got, rx, ru, P, "heterogeneous fleet random trajectory")
    assert np.all(got[0][:, 1 + 4] != ref[0][:, 1 + 4])                             # min_f follows each robot's own gain
    het.close()


def test_a_nan_stays_on_its_instance():
    eng, cst, batch, x, u, st, P = _solved("srbd13", 5, 1)
    own = _run(eng)
    bad = u.copy()
    bad[1, 2, 0] = np.nan                                                           # instance 1, node 2
    rec, nodes = _run(eng, x=x, u=bad)
    assert np.isnan(rec[1, :cc.COLS]).all() and rec[1, cc.LARGEST] == -1 and rec[1, cc.NODES] == eng.N
    assert np.isnan(nodes[1, 2]).all() and not np.isnan(np.delete(nodes[1], 2, axis=0)).any()
    keep = [0, 2, 3, 4, 5]
    assert rec[keep].tobytes() == own[0][keep].tobytes() and nodes[keep].tobytes() == own[1][keep].tobytes()


def test_nothing_else_moves():
    model, N, nb, M = "srbd13", 6, 5, 4
    batch = workload.make_batch(model, N, np.arange(nb) + 3)
    eng = DdpEngine(model, N, nb, opts=dict(OPTS, max_iters=2), consts=batch["consts"])
    eng.enable_resume()
    eng.enable_iteration_log(8)
    eng.enable_policy(M)
    solve(eng, batch)
    eng.policy_range_device()
    assert eng.unfinished() > 0                                                     # a cut solve: there are resume flags to keep

    def state():
        xs, us, stats = eng.fetch()
        rec, n = eng.iteration_log()
        return (xs.tobytes(), us.tobytes(), stats.tobytes(), eng.fetch_policy().tobytes(), eng.unfinished(), eng.unfinished(1, 3),
                rec.tobytes(), n.tobytes(), eng.queue_info(), eng.kernel_info())

    before = state()
    eng.cost_terms()
    _run(eng, 1, 3)
    _run(eng, x=batch["xs"], u=batch["us"])
    assert state() == before
    eng.close()
    # the class labels and their history of a handle that labels its instances itself
    eng = DdpEngine(model, N, nb, opts=dict(OPTS, queue_order=3), consts=batch["consts"])
    eng.enable_auto_classes()
    solve(eng, batch)
    labels = lambda: (eng._host_copy(_lib.BUF_CLASSES, "<i4").tobytes(), eng.auto_classes_info())      # noqa: E731
    before = labels()
    eng.cost_terms()
    _run(eng, x=batch["xs"], u=batch["us"])
    assert labels() == before
    eng.close()
    # the slots' work buffers: a forward after a backward, with and without the call between them
    eng = DdpEngine(model, N, nb, opts=dict(OPTS, max_iters=2), consts=batch["consts"])
    solve(eng, batch)
    eng.backward(batch["params"], 1e-6)
    ref = eng.forward(batch["params"], 0.5)
    eng.backward(batch["params"], 1e-6)
    eng.cost_terms()
    _run(eng, x=batch["xs"], u=batch["us"])
    got = eng.forward(batch["params"], 0.5)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(got, ref))
    eng.close()
    # a cut solve continued after the call is the one continued without it
    ends = []
    for call in (False, True):
        e = DdpEngine(model, N, nb, opts=dict(OPTS, max_iters=2), consts=batch["consts"])
        e.enable_resume()
        solve(e, batch)
        if call:
            e.cost_terms()
            _run(e, x=batch["xs"], u=batch["us"])
        e.set_options(max_iters=100)
        e.continue_solve()
        ends.append(tuple(a.tobytes() for a in e.fetch()))
        e.close()
    assert ends[0] == ends[1]


def test_refusals():
    model, N, nb = "srbd13", 6, 2
    batch = workload.make_batch(model, N, [0, 1])
    eng = DdpEngine(model, N, nb, opts=OPTS)
    with pytest.raises(RuntimeError, match="no solve has run"):
        eng.cost_terms()
    with pytest.raises(RuntimeError, match="no solve has run"):
        _run(eng)
    x, u, _ = solve(eng, batch)
    gx, gu = _dev(x), _dev(u)
    out = torch.zeros((nb, cc.WORDS), dtype=torch.float64, device="cuda")
    vp = eng._dev
    for dx, du in ((vp(gx, gx.shape), None), (None, vp(gu, gu.shape))):             # one of d_x / d_u NULL
        with pytest.raises(RuntimeError, match="both NULL"):
            eng._chk(eng.lib.sddp_cost_terms_range_device(eng.h, 0, nb, dx, du, vp(out, out.shape), None))
    with pytest.raises(RuntimeError, match="NULL argument"):
        eng._chk(eng.lib.sddp_cost_terms_range_device(eng.h, 0, nb, None, None, None, None))
    for call in (lambda: _run(eng, 1, 2), lambda: eng.cost_terms(1, 2), lambda: eng.cost_terms(-1, 1), lambda: eng.cost_terms(0, 0)):
        with pytest.raises(RuntimeError, match="range outside"):
            call()
    assert eng.lib.sddp_cost_terms_range_device(eng.h, 1, 2, None, None, vp(out, out.shape), None) == -1      # SDDP_ERR_ARG
    name = C.c_char_p()
    for family in (-1, cc.FAMILIES):
        assert eng.lib.sddp_cost_terms_name(family, C.byref(name)) == -1
        assert b"family must be 0 .. 12" in eng.lib.sddp_last_error(None)
    assert eng.cost_terms()["record"].shape == (nb, cc.WORDS)                       # and the handle still works
    eng.close()


def test_surface_and_fleet_queue():
    model, N, batch_n, depth = "srbd13", 6, 4, 2
    batch = workload.make_batch(model, N, np.arange(batch_n) + 3)
    eng = DdpEngine(model, N, batch_n * depth, opts=OPTS, consts=batch["consts"])
    words, families, name = C.c_int(), C.c_int(), C.c_char_p()
    eng._chk(eng.lib.sddp_cost_terms_words(eng.h, C.byref(words), C.byref(families)))
    assert (words.value, families.value) == (16, 13) == (cc.WORDS, cc.FAMILIES) == (_lib.COST_TERMS_WORDS, len(_lib.COST_TERM_NAMES))
    names = []
    for f in range(families.value):
        assert eng.lib.sddp_cost_terms_name(f, C.byref(name)) == 0
        names.append(name.value.decode())
    assert tuple(names) == _lib.COST_TERM_NAMES == cc.NAMES and len(set(names)) == 13
    t = {k: _dev(batch[k]) for k in ("x0", "xs", "us", "params")}
    fleet = FleetQueue(eng, t["params"].repeat(depth, 1, 1).contiguous(), batch_n, depth)
    out = torch.full((batch_n * depth + 1, cc.WORDS), 7.0, dtype=torch.float64, device="cuda")
    assert fleet.cost_terms(out) == 0                                               # nothing flushed yet: nothing launched
    fleet.submit(t["x0"], t["xs"], t["us"])
    assert fleet.flush() == batch_n and fleet.cost_terms(out) == batch_n            # a partial handle: the first block alone
    eng.synchronize()
    got = out.cpu().numpy()
    assert got[:batch_n].tobytes() == eng.cost_terms(0, batch_n)["record"].tobytes() and np.all(got[batch_n:] == 7.0)
    fleet.submit(t["x0"], t["xs"], t["us"])
    fleet.submit(t["x0"], t["xs"], t["us"])
    nd = torch.full((batch_n * depth, N + 1, cc.COLS), 7.0, dtype=torch.float64, device="cuda")
    assert fleet.flush() == batch_n * depth and fleet.cost_terms(out, nodes=nd) == batch_n * depth
    eng.synchronize()
    got = out.cpu().numpy()
    full = eng.cost_terms(nodes=True)
    assert got[:-1].tobytes() == full["record"].tobytes() and np.all(got[-1] == 7.0) and nd.cpu().numpy().tobytes() == full["nodes"].tobytes()
    assert got[:batch_n].tobytes() == got[batch_n:2 * batch_n].tobytes()            # the same robots in both blocks
    eng.close()
