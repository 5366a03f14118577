"""Constant sensitivities on the device (include/sddp.h sddp_const_gradient_range_device, sddp_const_gradient): the record and the per-node
addends of every model and build against the symbolic reference of tests/const_gradient_cases.py, assembled with the device's OWN
costates (d_lambda) on the device's own inputs.

Tolerance (const_gradient_cases.assert_result): every column, and every addend of it, within RTOL = 1e-11 -- the inspectors' tolerance --
of that column's magnitude sum  sum_k (|dL/dtheta| + sum_i |df/dtheta| |lambda|), formed by the reference.  The costates and words
34 - 36 are compared with sddp_stationarity_range_device's by their bits, the columns with the in-order sums of the addends by theirs.

The envelope check compares the chain rule's prediction D . delta with central differences of the converged cost of two further solves
with moved constants; its step and its bound come from the same experiment on the C oracle (const_gradient_cases.ENVELOPE_H,
ENVELOPE_DISCREPANCY; profiles/const_gradient/README.md).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from srbd_horizon_amd import _lib
from srbd_horizon_amd.engine import DdpEngine
from tests import consts_cases as kc, const_gradient_cases as cg, param_gradient_cases as pg, plan_audit_cases as pac
from tests.gpu_support import (COST_TERMS, STATIONARITY, Inspector, assert_a_nan_stays_on_its_instance, assert_a_user_build_is_refused,
                               assert_common_refusals, assert_fleet_queue_follows_the_last_flush, assert_nothing_else_moves,
                               assert_same_costates, run, touch_with)
from tests.gpu_support import engine_with_plan as _engine
from tests.variant_cases import draw

pytestmark = pytest.mark.gpu

OPTS = pac.OPTS


class _ConstGradient(Inspector):
    """the inspector as tests/gpu_support.py drives the others; DdpEngine.const_gradient returns (records, fields)"""
    __slots__ = ()

    def host(self, eng, first=0, count=None):
        return eng.const_gradient(first, count)[0]


CONST_GRADIENT = _ConstGradient("const_gradient", cg.W, dict(nodes=lambda e: (e.N + 1, cg.COLS), lam=lambda e: (e.N + 1, e.nx)),
                                lambda e, f, n, dx, du, out: e.lib.sddp_const_gradient_range_device(e.h, f, n, dx, du, out, None, None))


# (record [n, 40], addends [n, N + 1, 32], lambda [n, N + 1, nx]); lambda and words 34, 35, 36 are the stationarity certificate's
_run = functools.partial(run, CONST_GRADIENT)
_same_costates = functools.partial(assert_same_costates, (cg.LAM0, cg.STAT, cg.DEFECT))


def _check(model, csts, got, x, u, P, label):
    """csts: one RobotConsts, or one per instance"""
    rec, nodes, lam = got
    worst, refs = 0.0, []
    for b in range(rec.shape[0]):
        cst = csts[b] if isinstance(csts, (list, tuple)) else csts
        th = cg.derived(cg.library_consts(model, cst))
        ref = cg.reference(cg.gradients(model, cst), th, x[b], u[b], P[b], lam[b])
        worst = max(worst, cg.assert_result(rec[b], nodes[b], ref, th, f"{label} instance {b}"))
        refs.append(ref)
    print(f"{label}: worst error / tolerance {worst:.3e}")
    return refs


def _consts(model, key):
    return kc.defaults(model) if key == "default" else dict(kc.ALL_OFF[model])


@pytest.mark.parametrize("N", (1, 2, 65))
@pytest.mark.parametrize("key", ("default", "off"))
@pytest.mark.parametrize("model", cg.MODELS)
def test_knot_level_parity(model, key, N):
    """a random, non-converged caller trajectory (open gaps, generic lambda), random parameters with switches at 0 and 1; N = 1: one stage
    node and the terminal node, N = 65: 66 nodes over 64 lanes"""
    B = 3
    batch, x, u, P = pg.random_plan(model, N, B, seed=7)
    consts = _consts(model, key)
    cst = kc.oracle_consts(model, consts)
    eng = _engine(model, N, B, consts, P, batch)
    got = _run(eng, x=x, u=u)
    _check(model, cst, got, x, u, P, f"{model} {key} N = {N}")
    _same_costates(eng, got, x, u)
    rec, nodes, _ = got
    dead = cg.zero_columns(model)
    assert np.all(rec[:, dead] == 0.0) and np.all(nodes[:, :, dead] == 0.0)      # what the model does not read: exact zeros
    # (w_sw is felt only where a switch is off: left out, a short horizon may have none)
    live = [c for c in range(cg.COLS) if c not in dead and c != cg.COL["w_sw"]]
    assert np.all(np.any(nodes[:, :, live] != 0.0, axis=1))                      # and everything it reads is felt
    assert np.all(rec[:, cg.NODES] == N)
    eng.close()


def test_range_plan_source_and_the_python_surface():
    model, N, B = "srbd13", 6, 3
    batch, _, _, P = pg.random_plan(model, N, B, seed=3)
    eng = _engine(model, N, B, batch["consts"], batch["params"], batch, solve_it=True)
    x, u, _ = eng.fetch()
    cst = kc.oracle_consts(model, batch["consts"])
    own = _run(eng)
    _check(model, cst, own, x, u, batch["params"], "srbd13 solved plan")
    _same_costates(eng, own)
    part = _run(eng, 1, 1)                                                      # the range [1, 2) is row 1 of the full call
    assert all(a.tobytes() == b_[1:2].tobytes() for a, b_ in zip(part, own))
    same = _run(eng, x=x, u=u)                                                  # the handle's own plan as a caller's trajectory
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(same, own))
    part = _run(eng, 1, 2, x=x[1:3], u=u[1:3])                                  # block i is instance first + i
    assert all(a.tobytes() == b_[1:3].tobytes() for a, b_ in zip(part, own))
    assert _run(eng, full=False)[0].tobytes() == own[0].tobytes()               # d_nodes / d_lambda NULL
    # the host twin and the Python surface
    rec = np.empty((B, cg.W))
    eng._chk(eng.lib.sddp_const_gradient(eng.h, 0, B, _lib.ptr(rec)))
    assert rec.tobytes() == own[0].tobytes()
    record, fields, nodes = eng.const_gradient(nodes=True)
    assert record.tobytes() == own[0].tobytes() and nodes.tobytes() == own[1].tobytes() and len(fields) == B
    th = cg.derived(batch["consts"])
    for b in range(B):
        want, mag = cg.fields_of(batch["consts"], own[0][b, :cg.COLS])
        flat = np.concatenate([np.atleast_1d(fields[b][n]) for n in ("m", "I", "com", "feet")] +
                              [[fields[b][n] for n in cg.FIELD_NAMES[25:]]])
        assert flat.shape == (41,) and np.all(np.abs(flat - want) <= cg.FIELDS_RTOL * mag)
        assert np.isclose(fields[b]["m"], -th[1] / batch["consts"]["m"] * own[0][b, 1], rtol=1e-14)     # -force_scaling / m^2 C[inv_ms]
    words, cols = C.c_int(), C.c_int()
    eng._chk(eng.lib.sddp_const_gradient_words(eng.h, C.byref(words), C.byref(cols)))
    assert (words.value, cols.value) == (40, 32)
    eng.close()


def test_instance_constants():
    """two robots (and a third) with their own m, I, dt and gains: instance b matches the reference built with its own robot, and not the
    handle's; a table whose rows equal the handle's constants gives the plain form's bits"""
    model, N, B = "srbd13", 4, 3
    batch, x, u, P = pg.random_plan(model, N, B, seed=11)
    over, csts = draw(batch["consts"], B, ("dt", "r_tracking_gain", "rdot_tracking_gain", "w_tracking_gain", "min_qddot_gain",
                                           "force_switch_weight", "min_f_gain"), seed=3)
    plain = _engine(model, N, B, batch["consts"], P, batch)
    ref = _run(plain, x=x, u=u)
    eng = DdpEngine(model, N, B, opts=dict(OPTS, max_iters=0), consts=batch["consts"])
    eng.set_instance_consts(dict(m=np.full(B, eng.consts.m)))                    # a table equal to the handle's constants
    assert eng.instance_consts_active()
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(P)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(_run(eng, x=x, u=u), ref))
    eng.set_instance_consts(over)
    got = _run(eng, x=x, u=u)
    refs = _check(model, csts, got, x, u, P, "heterogeneous fleet")
    common = kc.oracle_consts(model, batch["consts"])
    for b in range(B):
        th = cg.derived(cg.library_consts(model, common))
        other = cg.reference(cg.gradients(model, common), th, x[b], u[b], P[b], got[2][b])
        miss = np.max(np.abs(got[0][b, :cg.COLS] - other[1]) / np.where(refs[b][2] > 0, refs[b][2], np.inf))
        assert miss > 1e3 * cg.RTOL, f"robot {b}: the handle's own robot would do as well ({miss:.3e})"
        # the chain rule runs through the robot's own constants
        fields = eng.const_gradient_fields(got[0][b], b)
        assert np.isclose(fields["m"], -csts[b].force_scaling / csts[b].m**2 * got[0][b, 1], rtol=1e-14)
    eng.close()
    plain.close()


@pytest.mark.parametrize("kind", ("x", "bar", "box", "so2"))
def test_builds(kind):
    """the _x build, the friction and the bound barrier builds and the second_order = 2 build of srbd13: the barrier columns against the
    reference on the barrier builds, exact zeros elsewhere"""
    model, N, B = "srbd13", 6, 3
    batch, P, consts, opts = pac.problem(model, N, B, kind)
    rng = np.random.default_rng(5)
    x = batch["xs"] + 0.05 * rng.standard_normal(batch["xs"].shape)
    u = batch["us"] + 0.05 * rng.standard_normal(batch["us"].shape)
    eng = DdpEngine(model, N, B, opts=dict(opts, max_iters=0), consts=consts)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(P)
    got = _run(eng, x=x, u=u)
    cst = kc.oracle_consts(model, {k: v for k, v in consts.items() if k != "extra_rows"})
    _check(model, cst, got, x, u, P, f"srbd13 {kind}")
    _same_costates(eng, got, x, u)
    rec, nodes, _ = got
    dead = cg.zero_columns(model, kind == "bar", kind == "box")
    assert np.all(rec[:, dead] == 0.0) and np.all(nodes[:, :, dead] == 0.0)
    on = [cg.COL[n] for n in (cg.FRICTION_COLS if kind == "bar" else cg.BOUND_COLS if kind == "box" else ())]
    assert np.all(rec[:, on] != 0.0)
    # (an _x build's rows read no constant of a column, but they move the costates, and through them the columns that enter f)
    eng.close()


def test_cross_check_with_the_cost_breakdown():
    """L is linear in every gain and f reads none: C[w] w is the cost of the family that gain weighs (sddp_cost_terms), for every gain > 0,
    within RTOL of the column's magnitude sum times the gain"""
    pairs = {"r_tracking": ("w_rz", "w_rxy"), "rdot_tracking": ("w_rd",), "w_tracking": ("w_w",), "rel_pos": ("w_rel",), "min_f": ("w_f",),
             "force_switch": ("w_sw",), "min_qddot": ("gq",), "zmp_tracking": ("w_zmp",), "friction_barrier": ("bar_w",), "bound_barrier": ("box_w",)}
    for model, kind in (("srbd13", "plain"), ("srbd37", "plain"), ("lip30", "plain"), ("srbd61", "plain"), ("srbd13", "bar"), ("srbd13", "box")):
        N, B = 5, 2
        batch, P, consts, opts = pac.problem(model, N, B, kind)
        rng = np.random.default_rng(9)
        x = batch["xs"] + 0.05 * rng.standard_normal(batch["xs"].shape)
        u = batch["us"] + 0.05 * rng.standard_normal(batch["us"].shape)
        eng = _engine(model, N, B, consts, P, batch, opts={k: v for k, v in opts.items() if k not in OPTS})
        got = _run(eng, x=x, u=u)
        terms = COST_TERMS.device(eng, x=x, u=u)[0]
        cst = kc.oracle_consts(model, consts)
        th = cg.derived(cg.library_consts(model, cst))
        checked = 0
        for b in range(B):
            mag = cg.reference(cg.gradients(model, cst), th, x[b], u[b], P[b], got[2][b])[2]
            for family, cols in pairs.items():
                cols = [cg.COL[c] for c in cols]
                if not all(th[c] > 0.0 for c in cols) or any(c in cg.zero_columns(model, kind == "bar", kind == "box") for c in cols[:1]):
                    continue
                mine = sum(got[0][b, c] * th[c] for c in cols)
                fam = terms[b, 1 + _lib.COST_TERM_NAMES.index(family)]
                tol = cg.RTOL * sum(mag[c] * th[c] for c in cols)
                assert abs(mine - fam) <= tol, f"{model} {kind} instance {b} {family}: {mine} against {fam}, tolerance {tol:.3e}"
                checked += 1
        assert checked >= B * (5 if model == "lip30" else 6)
        eng.close()


def test_a_user_build_is_refused():
    assert_a_user_build_is_refused(CONST_GRADIENT, "no derivative code")


def test_a_horizon_past_the_lds_limit_is_refused():
    """the tile of addends is (N + 2) * 256 bytes: N = 254 is the last that fits the 64 KB of a workgroup, N = 255 is refused before
    anything is launched"""
    from srbd_horizon_amd import workload
    model, B = "srbd13", 1
    for N, fits in ((254, True), (255, False)):
        batch = workload.make_batch(model, N, [0])
        eng = _engine(model, N, B, batch["consts"], batch["params"], batch)
        out = torch.full((B, cg.W), 7.0, dtype=torch.float64, device="cuda")
        if fits:
            eng.const_gradient_device(out)
            eng.synchronize()
            assert out.cpu().numpy()[0, cg.NODES] == N
        else:
            with pytest.raises(RuntimeError, match="bytes of LDS"):
                eng.const_gradient_device(out)
            eng.synchronize()
            assert np.all(out.cpu().numpy() == 7.0)
            assert STATIONARITY.device(eng)[0].shape == (B, 8)
        eng.close()


def test_a_nan_stays_on_its_instance():
    assert_a_nan_stays_on_its_instance(CONST_GRADIENT, pg.random_plan, cg.REL, (cg.COLUMN,), cg.NODES)


def test_envelope_of_the_optimal_cost():
    """srbd13, N = 8, B = 4, tight options: at a converged plan with closed gaps D . delta -- D the record carried to the fields by
    sddp_const_gradient_fields with the handle's constants, delta a direction over m, I, dt, rdot_tracking_gain and min_f_gain -- is the
    derivative of the OPTIMAL cost along delta, against (J*(+h) - J*(-h)) / 2h from two further solves on handles made with the moved
    constants.  h = 1e-4 is the step at which the same experiment with the C oracle's solves and the symbolic reference has its smallest
    discrepancy, 2.35e-9 of sum |D delta| (tests/test_const_gradient_cpu.py measures both again); the device is allowed 10 x that,
    2.35e-8, the margin the parameter sensitivities took over their CPU figure.  All four robots, all three solves."""
    assert (cg.ENVELOPE_H, cg.ENVELOPE_DISCREPANCY) == (1e-4, 2.35e-9)
    batch, delta = cg.envelope_problem()
    P, h = batch["params"], cg.ENVELOPE_H
    B = P.shape[0]
    assert B == 4

    def converged(consts, xs, us, inspect=False):
        eng = DdpEngine(pg.ENVELOPE_MODEL, pg.ENVELOPE_N, B, opts=pg.ENVELOPE_OPTS, consts=consts)
        eng.load(batch["x0"], xs, us)
        x, u = eng.solve(P)
        st = eng.stats
        assert st["converged"].all() and (st["status"] == 0).all() and (st["gap"] <= pg.ENVELOPE_GAP).all(), st
        got = eng.const_gradient() if inspect else None
        eng.close()
        return x.copy(), u.copy(), st["cost"].copy(), got

    x, u, _, (rec, fields) = converged(batch["consts"], batch["xs"], batch["us"], inspect=True)
    D = np.stack([cg.flat_of_field_dict(f) for f in fields])
    Jp, Jm = (converged(cg.moved_consts(batch["consts"], delta, s * h), x, u)[2] for s in (1.0, -1.0))
    d = cg.envelope_discrepancy(D, delta, Jp, Jm, h)
    print(f"envelope: discrepancy per robot {d}, bound {10.0 * cg.ENVELOPE_DISCREPANCY:.3e}; "
          f"stationarity (word 35) of the base plans {rec[:, cg.STAT]}, defect {rec[:, cg.DEFECT]}")
    assert (d <= 10.0 * cg.ENVELOPE_DISCREPANCY).all(), d


def test_nothing_else_moves():
    assert_nothing_else_moves(touch_with(CONST_GRADIENT), OPTS)


def test_refusals():
    assert_common_refusals(CONST_GRADIENT, OPTS)


def test_fleet_queue_follows_the_last_flushed_range():
    assert_fleet_queue_follows_the_last_flush(CONST_GRADIENT, OPTS, "nodes")[0].close()
