"""Cost breakdown on the device (include/sddp.h sddp_cost_terms_range_device, sddp_cost_terms): the record and the per-node addends of
every kernel family and build kind against statement A of tests/cost_terms_cases.py (the oracle's cost with the gains masked family
by family) on the device's own fetched x, u, P, and what the record promises exactly.

Tolerance (cost_terms_cases.tolerances): per family, 64 x the A-versus-B disagreement of the two CPU statements committed in
profiles/cost_terms/cpu_disagreement.json, relative to the record's word; a family on which the two CPU statements agree to less than
one rounding (they share the rows' values sqrt(w) e and differ in the order of one sum only) is given 64 x eps, since the device forms
w e^2 where both of them form (sqrt(w) e)^2.  Every test prints its worst |difference| / tolerance.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import models as omodels
from srbd_horizon_amd import _lib, workload
from srbd_horizon_amd.engine import DdpEngine
from tests import cost_terms_cases as cc
from tests.gpu_support import (BUILDS, COST_TERMS, assert_common_refusals, assert_fleet_queue_follows_the_last_flush,
                               assert_nothing_else_moves, solve, solved, touch_with)
from tests.variant_cases import SRBD13_FIELDS, draw

pytestmark = pytest.mark.gpu

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
B = 6
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cost_terms", "cpu_disagreement.json")) as _f:
    TOL = cc.tolerances(json.load(_f))
FAM = slice(1, 1 + cc.FAMILIES)


def _run(eng, first=0, count=None, x=None, u=None, nodes=True):
    """cost_terms_device on fresh device tensors -> numpy (record [n, 16], addends [n, N + 1, 14] or None)"""
    return COST_TERMS.device(eng, first, count, x, u, optional=nodes)


def _solved(model, N, wps=1, kind="plain"):
    """the case on the seeds 3 .. B + 2; "x" here: the rows of tests/cost_terms_cases.py ("lin" of plan_audit_cases.problem)"""
    return solved(model, N, B, "lin" if kind == "x" else kind, wps=wps)


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
    assert_nothing_else_moves(touch_with(COST_TERMS), OPTS)


def test_refusals():
    assert_common_refusals(COST_TERMS, OPTS)
    lib, name = _lib.load(), C.c_char_p()
    for family in (-1, cc.FAMILIES):
        assert lib.sddp_cost_terms_name(family, C.byref(name)) == -1
        assert b"family must be 0 .. 12" in lib.sddp_last_error(None)


def test_surface_and_fleet_queue():
    eng = DdpEngine("srbd13", 6, 2, opts=OPTS)
    words, families, name = C.c_int(), C.c_int(), C.c_char_p()
    eng._chk(eng.lib.sddp_cost_terms_words(eng.h, C.byref(words), C.byref(families)))
    assert (words.value, families.value) == (16, 13) == (cc.WORDS, cc.FAMILIES) == (_lib.COST_TERMS_WORDS, len(_lib.COST_TERM_NAMES))
    names = []
    for f in range(families.value):
        assert eng.lib.sddp_cost_terms_name(f, C.byref(name)) == 0
        names.append(name.value.decode())
    assert tuple(names) == _lib.COST_TERM_NAMES == cc.NAMES and len(set(names)) == 13
    eng.close()
    assert_fleet_queue_follows_the_last_flush(COST_TERMS, OPTS, "nodes")[0].close()
