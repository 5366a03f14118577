"""Parameter sensitivities on the device (include/sddp.h sddp_param_gradient_range_device, sddp_param_gradient): the gradient and the
record of every model, of the "_x", a barrier and the second_order = 2 build against the symbolic reference of
tests/param_gradient_cases.py, assembled with the device's OWN costates (d_lambda) on the device's own inputs.

Tolerance (param_gradient_cases.assert_result): every entry of G and words 0, 3 within RTOL = 1e-11 -- the relative tolerance of g and F
in tests/test_gpu_parity.py test_eval_knots_matches_oracle -- of the instance's word 3.  The costates and words 4 - 6 are compared with
sddp_stationarity_range_device's by their bits.

The envelope check compares sum G . dp with central differences of the converged cost of two further solves; its step and its bound
come from the same experiment on the C oracle (param_gradient_cases.ENVELOPE_H, ENVELOPE_DISCREPANCY; profiles/param_gradient/README.md).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from srbd_horizon_amd import _lib
from srbd_horizon_amd.engine import DdpEngine
from tests import param_gradient_cases as pg, plan_audit_cases as pac
from tests.gpu_support import (Inspector, assert_a_nan_stays_on_its_instance, assert_a_user_build_is_refused, assert_common_refusals,
                               assert_fleet_queue_follows_the_last_flush, assert_nothing_else_moves, assert_same_costates, run, touch_with)
from tests.gpu_support import engine_with_plan as _engine
from tests.variant_cases import TRACKING, draw

pytestmark = pytest.mark.gpu

OPTS = pac.OPTS


class _ParamGradient(Inspector):
    """the inspector as tests/gpu_support.py drives the others; its host twin takes the optional gradient behind the records"""
    __slots__ = ()

    def host(self, eng, first=0, count=None):
        n = eng.B - first if count is None else count
        out = np.empty((max(n, 0), self.words))
        eng._chk(eng.lib.sddp_param_gradient(eng.h, int(first), int(n), _lib.ptr(out), None))
        return out


PARAM_GRADIENT = _ParamGradient("param_gradient", pg.W, dict(grad=lambda e: (e.N + 1, e.np_), lam=lambda e: (e.N + 1, e.nx)),
                                lambda e, f, n, dx, du, out: e.lib.sddp_param_gradient_range_device(e.h, f, n, dx, du, out, None, None))


# (record [n, 8], G [n, N + 1, np], lambda [n, N + 1, nx]); lambda and words 4, 5, 6 are the stationarity certificate's
_run = functools.partial(run, PARAM_GRADIENT)
_same_costates = functools.partial(assert_same_costates, (pg.LAM0, pg.STAT, pg.DEFECT))


def _check(J, got, x, u, P, label):
    rec, G, lam = got
    worst = 0.0
    for b in range(rec.shape[0]):
        worst = max(worst, pg.assert_result(rec[b], G[b], pg.reference(J, x[b], u[b], P[b], lam[b]), f"{label} instance {b}"))
        assert rec[b, pg.NODES] == u.shape[1]
    print(f"{label}: worst error / tolerance {worst:.3e}")


@pytest.mark.parametrize("N", (1, 2, 65))
@pytest.mark.parametrize("key", ("default", "off"))
@pytest.mark.parametrize("model", pg.MODELS)
def test_knot_level_parity(model, key, N):
    """a random, non-converged caller trajectory (open gaps, generic lambda), random parameters with switches at 0 and 1; N = 1: a
    terminal and one stage node, N = 65: one node past a wavefront"""
    B = 3
    batch, x, u, P = pg.random_plan(model, N, B, seed=7)
    consts = dict(batch["consts"], **pg.CONSTS[key])
    J = pg.jacobians(model, pg.register(f"{model}:{key}", consts))
    eng = _engine(model, N, B, consts, P, batch)
    got = _run(eng, x=x, u=u)
    _check(J, got, x, u, P, f"{model} {key} N = {N}")
    _same_costates(eng, got, x, u)
    if model == "srbd13":
        assert np.any(got[1][:, :N, 11:17] != 0.0)          # the footholds are felt on the stage nodes, through f as well
    eng.close()


def test_range_and_plan_source():
    model, N, B = "srbd13", 6, 3
    batch, _, _, P = pg.random_plan(model, N, B, seed=3)
    eng = _engine(model, N, B, batch["consts"], batch["params"], batch, solve_it=True)
    x, u, _ = eng.fetch()
    own = _run(eng)
    _check(pg.jacobians(model, pg.register("srbd13:batch", batch["consts"])), own, x, u, batch["params"], "srbd13 solved plan")
    _same_costates(eng, own)
    part = _run(eng, 1, 2)                                                      # the range is rows 1 .. 2 of the full call
    assert all(a.tobytes() == b_[1:3].tobytes() for a, b_ in zip(part, own))
    same = _run(eng, x=x, u=u)                                                  # the handle's own plan as a caller's trajectory
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(same, own))
    part = _run(eng, 1, 2, x=x[1:3], u=u[1:3])                                  # block i is instance first + i
    assert all(a.tobytes() == b_[1:3].tobytes() for a, b_ in zip(part, own))
    assert _run(eng, full=False)[0].tobytes() == own[0].tobytes()               # d_grad / d_lambda NULL
    # the host twins and the Python surface
    assert PARAM_GRADIENT.host(eng).tobytes() == own[0].tobytes() and PARAM_GRADIENT.host(eng, 1, 2).tobytes() == own[0][1:3].tobytes()
    rec, G = np.empty((B, pg.W)), np.empty((B, N + 1, eng.np_))
    eng._chk(eng.lib.sddp_param_gradient(eng.h, 0, B, _lib.ptr(rec), _lib.ptr(G)))
    assert rec.tobytes() == own[0].tobytes() and G.tobytes() == own[1].tobytes()
    grad, record, lam = eng.param_gradient(want_lambda=True)
    eng.synchronize()
    assert all(t.cpu().numpy().tobytes() == a.tobytes() for t, a in zip((record, grad, lam), own))
    words, width = C.c_int(), C.c_int()
    eng._chk(eng.lib.sddp_param_gradient_words(eng.h, C.byref(words), C.byref(width)))
    assert (words.value, width.value) == (8, 19)
    eng.close()


def test_instance_constants():
    """every robot its own: instance b matches the reference built with its own robot"""
    model, N, B = "srbd13", 4, 3
    batch, x, u, P = pg.random_plan(model, N, B, seed=11)
    over, csts = draw(batch["consts"], B, TRACKING + ("min_qddot_gain", "force_switch_weight"), seed=3)
    eng = DdpEngine(model, N, B, opts=dict(OPTS, max_iters=0), consts=batch["consts"])
    eng.set_instance_consts(over)
    assert eng.instance_consts_active()
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(P)
    got = _run(eng, x=x, u=u)
    common = pg.jacobians(model, pg.register("srbd13:batch11", batch["consts"]))
    for b in range(B):
        J = pg.jacobians(model, pg.register(f"srbd13:robot{b}", csts[b]))
        _check(J, tuple(a[b:b + 1] for a in got), x[b:b + 1], u[b:b + 1], P[b:b + 1], f"robot {b}")
        miss = np.max(np.abs(got[1][b] - pg.reference(common, x[b], u[b], P[b], got[2][b])[0])) / got[0][b, pg.SCALE]
        assert miss > 1e3 * pg.RTOL, f"robot {b}: the handle's own robot would do as well ({miss:.3e})"
    eng.close()


@pytest.mark.parametrize("kind", ("x", "bar", "so2"))
def test_builds(kind):
    """the _x build (linear user rows: the row is np + 8 wide and the reference columns are -2 w e), a barrier build and the
    second_order = 2 build of srbd13"""
    model, N, B = "srbd13", 6, 3
    batch, P, consts, opts = pac.problem(model, N, B, kind)
    rng = np.random.default_rng(5)
    x = batch["xs"] + 0.05 * rng.standard_normal(batch["xs"].shape)
    u = batch["us"] + 0.05 * rng.standard_normal(batch["us"].shape)
    if kind == "x":
        P = P.copy()
        P[:, :, 19:] += 0.1 * rng.standard_normal((B, N + 1, 8))
    eng = DdpEngine(model, N, B, opts=dict(opts, max_iters=0), consts=consts)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(P)
    words, width = C.c_int(), C.c_int()
    eng._chk(eng.lib.sddp_param_gradient_words(eng.h, C.byref(words), C.byref(width)))
    assert (words.value, width.value, eng.np_) == (8, 27 if kind == "x" else 19, 27 if kind == "x" else 19)
    got = _run(eng, x=x, u=u)
    _check(pg.jacobians(model, pg.register(f"srbd13:{kind}", consts)), got, x, u, P, f"srbd13 {kind}")
    _same_costates(eng, got, x, u)
    if kind == "x":
        rows = consts["extra_rows"]
        G = got[1]
        assert np.all(G[:, :, 19 + len(rows):] == 0.0)                          # rows not in use
        for j, row in enumerate(rows):                                          # -2 w (a . z - (p_ref + const)) where the kind is active
            for k in range(N + 1):
                on = k >= 1 if row["kind"] == "state" else k < N
                z = np.concatenate([x[:, k], u[:, k] if k < N else np.zeros((B, eng.nu))], axis=1)
                want = -2.0 * row["w"] * (z @ row["a"] - P[:, k, 19 + j] - row["const"]) if on else np.zeros(B)
                assert np.allclose(G[:, k, 19 + j], want, rtol=1e-12, atol=1e-12 * max(1.0, row["w"]))
    eng.close()


def test_nothing_else_moves():
    assert_nothing_else_moves(touch_with(PARAM_GRADIENT), OPTS)


def test_a_nan_stays_on_its_instance():
    assert_a_nan_stays_on_its_instance(PARAM_GRADIENT, pg.random_plan, pg.GRAD, (pg.NODE, pg.COLUMN), pg.NODES)


def test_refusals():
    assert_common_refusals(PARAM_GRADIENT, OPTS)


def test_a_user_build_is_refused():
    assert_a_user_build_is_refused(PARAM_GRADIENT, "no derivative in the parameters")


def test_envelope_of_the_optimal_cost():
    """srbd13, N = 8, B = 4, tight options: at a converged plan with closed gaps sum G . dp is the derivative of the OPTIMAL cost along
    dp (rdot_ref and the footholds of every node), against (J*(p + h dp) - J*(p - h dp)) / 2h from two further solves.  h = 1e-5 is
    the step at which the same experiment with the C oracle's solves and the symbolic reference has its smallest discrepancy, 8.03e-9
    of sum |G . dp| (tests/test_param_gradient_cpu.py measures both again); the device is allowed 10 x that, 8.03e-8, because its end
    point differs from the oracle's by up to the parity tolerance of converged solves.  All four robots, all three solves."""
    assert (pg.ENVELOPE_H, pg.ENVELOPE_DISCREPANCY) == (1e-5, 8.03e-9)
    batch, dP = pg.envelope_problem()
    P, h = batch["params"], pg.ENVELOPE_H
    B = P.shape[0]
    assert B == 4
    eng = DdpEngine(pg.ENVELOPE_MODEL, pg.ENVELOPE_N, B, opts=pg.ENVELOPE_OPTS, consts=batch["consts"])

    def converged(params, xs, us):
        eng.load(batch["x0"], xs, us)
        x, u = eng.solve(params)
        st = eng.stats
        assert st["converged"].all() and (st["status"] == 0).all() and (st["gap"] <= pg.ENVELOPE_GAP).all(), st
        return x.copy(), u.copy(), st["cost"].copy()

    x, u, _ = converged(P, batch["xs"], batch["us"])
    rec, G, _ = _run(eng)
    Jp, Jm = (converged(P + s * h * dP, x, u)[2] for s in (1.0, -1.0))
    d = pg.envelope_discrepancy(G, dP, Jp, Jm, h)
    print(f"envelope: discrepancy per robot {d}, bound {10.0 * pg.ENVELOPE_DISCREPANCY:.3e}; "
          f"stationarity (word 5) of the base plans {rec[:, pg.STAT]}, defect {rec[:, pg.DEFECT]}")
    assert (d <= 10.0 * pg.ENVELOPE_DISCREPANCY).all(), d
    eng.close()


def test_fleet_queue_follows_the_last_flushed_range():
    assert_fleet_queue_follows_the_last_flush(PARAM_GRADIENT, OPTS, "grad")[0].close()
