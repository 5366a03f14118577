"""Constant sensitivities (include/sddp.h sddp_const_gradient_range_device), what needs no GPU: the host chain rule
sddp_const_gradient_fields and the name tables of the library, and the symbolic reference of tests/const_gradient_cases.py against
central differences of the C oracle's f and L with one derived constant perturbed.

CENTRAL DIFFERENCES, one column at a time.  The oracle takes sddp_model_consts' fields, so column c of theta moves through the robot
whose derived record is theta + h e_c (consts_of_derived: force_scaling kept, m = force_scaling / inv_ms, I = force_scaling Is,
lip_height = g / eta2, ...).  w_rz and w_rxy are one field (r_tracking_gain): they move together and the SUM of the two columns is
checked.  L is a polynomial of degree <= 2 in the gains, com_z, the offsets, inv_ms and eta2 and f affine in dt, inv_ms and eta2, where a
central difference has no truncation error; in Is (through the inverse of the world inertia) and in the barrier constants it has.  The
truncation error of the quotient D(h) is taken from the oracle itself, by Richardson: D(2h) - D(h) = 3 x it to leading order, so
    tolerance = 2 |D(2h) - D(h)| / 3  +  E eps |L0| / h  +  E eps (|reference| + 1),        h = 1e-3 |theta_c| (1e-3 where that is 0),
E = 64 the project's margin for two correct float64 statements of one sum (tests/stationarity_cases.py MARGIN); for f the same with
max |f| in place of |L0|.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import cport
from srbd_horizon_amd import _lib
from tests import consts_cases as kc, const_gradient_cases as cg, param_gradient_cases as pg

EPS = np.finfo(np.float64).eps
E = 64.0
SETS = ("default", "off")


def _consts(model, key):
    return kc.defaults(model) if key == "default" else dict(kc.ALL_OFF[model])


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _fields(lib, consts_struct, derived):
    out, n = np.full(64, 7.0), C.c_int()
    rc = lib.sddp_const_gradient_fields(C.byref(consts_struct), _lib.ptr(np.ascontiguousarray(derived, dtype=float)), _lib.ptr(out), C.byref(n))
    return rc, out, n.value, (lib.sddp_last_error(None) or b"").decode()


def test_the_name_tables(lib):
    name = C.c_char_p()
    cols = []
    while lib.sddp_const_gradient_name(len(cols), C.byref(name)) == 0:
        cols.append(name.value.decode())
    assert tuple(cols) == cg.NAMES == _lib.CONST_GRADIENT_NAMES and len(cols) == _lib.CONST_GRADIENT_COLS == 32
    fields = []
    while lib.sddp_const_gradient_field_name(len(fields), C.byref(name)) == 0:
        fields.append(name.value.decode())
    assert tuple(fields) == cg.FIELD_NAMES == _lib.CONST_GRADIENT_FIELD_NAMES and len(fields) == 41
    for fn, n in ((lib.sddp_const_gradient_name, 32), (lib.sddp_const_gradient_field_name, 41)):
        assert fn(-1, C.byref(name)) == -1 and fn(n, C.byref(name)) == -1 and fn(0, None) == -1
    # every field is a field of sddp_model_consts
    c = _lib.default_consts("srbd13")
    assert all(hasattr(c, f.partition("[")[0]) for f in fields)
    assert _lib.CONST_GRADIENT_WORDS == 40 and len(_lib.CONST_GRADIENT_TAIL) == 8


@pytest.mark.parametrize("key", SETS)
@pytest.mark.parametrize("model", cg.MODELS)
def test_fields_against_central_differences_of_make_dev_consts(lib, model, key):
    consts = _consts(model, key)
    consts.update(friction_cone_coefficient=0.6, friction_barrier_weight=2.0, friction_barrier_sharpness=4.0)      # (host code: any build's constants)
    struct = _lib.default_consts(model, **consts)
    rng = np.random.default_rng(11)
    worst = 0.0
    for trial in range(3):
        Cd = rng.standard_normal(32) * 10.0 ** rng.uniform(-3, 3, 32)
        rc, out, n, msg = _fields(lib, struct, Cd)
        assert rc == 0 and n == 41 and np.all(out[41:] == 7.0), msg
        want, mag = cg.fields_of(consts, Cd)
        err = np.abs(out[:41] - want)
        assert np.all(err <= cg.FIELDS_RTOL * mag), [(cg.FIELD_NAMES[i], out[i], want[i]) for i in np.nonzero(err > cg.FIELDS_RTOL * mag)[0]]
        worst = max(worst, float(np.max(err[mag > 0] / (cg.FIELDS_RTOL * mag[mag > 0]))))
        silent = [i for i, f in enumerate(cg.FIELD_NAMES) if f in ("com[0]", "com[1]") or (f.startswith("feet") and int(f[5:-1]) % 3 == 2)
                  or f in ("feet[2]", "feet[5]", "feet[8]", "feet[11]")]
        assert np.all(out[silent] == 0.0)
    print(f"{model} {key}: worst error / tolerance {worst:.3e}")
    # the documented formulas, spelled out once
    Cd = np.zeros(32); Cd[cg.COL["inv_ms"]] = 1.0
    out = _fields(lib, struct, Cd)[1]
    assert np.isclose(out[0], -struct.force_scaling / struct.m**2, rtol=1e-15) and np.isclose(out[26], 1.0 / struct.m, rtol=1e-15)
    Cd = np.zeros(32); Cd[cg.COL["w_rz"]], Cd[cg.COL["w_rxy"]] = 2.0, 3.0
    assert _fields(lib, struct, Cd)[1][27] == 5.0


def test_fields_refusals(lib):
    good = _lib.default_consts("srbd13")
    Cd = np.ones(32)
    out, n = np.zeros(41), C.c_int()
    assert lib.sddp_const_gradient_fields(None, _lib.ptr(Cd), _lib.ptr(out), C.byref(n)) == -1 and n.value == 41
    assert lib.sddp_const_gradient_fields(C.byref(good), None, _lib.ptr(out), None) == -1
    assert lib.sddp_const_gradient_fields(C.byref(good), _lib.ptr(Cd), None, None) == -1
    for field, value, msg in (("m", float("nan"), "m must be finite and > 0"), ("m", float("inf"), "m must be finite and > 0"),
                              ("force_scaling", 0.0, "force_scaling must be finite and > 0"), ("lip_height", -1.0, "lip_height must be finite and > 0"),
                              ("min_f_gain", -1.0, "min_f_gain must be finite and >= 0"), ("lever_sign", 0.5, "lever_sign must be +1 or -1")):
        bad = _lib.default_consts("srbd13")
        setattr(bad, field, value)
        rc, _, _, err = _fields(lib, bad, Cd)
        assert rc == -1 and err == msg, (field, err)
    assert _fields(lib, good, Cd)[0] == 0


# ---- the symbolic reference against the C oracle ---------------------------------------------------------------------------------------------
def consts_of_derived(model, cst, th):
    """the RobotConsts whose derived record is th (force_scaling kept; w_rz = w_rxy = th[w_rz] is the one r_tracking_gain)"""
    fs = cst.force_scaling
    feet = np.array(cst.feet8 if model == "srbd61" else cst.feet, dtype=float)
    feet[2, 0:2] = feet[0, 0:2] + th[[cg.COL["d1x"], cg.COL["d1y"]]]
    feet[3, 0:2] = feet[1, 0:2] + th[[cg.COL["d2x"], cg.COL["d2y"]]]
    com = np.array(cst.com, dtype=float); com[2] = th[cg.COL["com_z"]]
    return dataclasses.replace(
        cst, dt=th[0], m=fs / th[1], I=fs * th[2:11].reshape(3, 3), com=com, r_tracking_gain=th[cg.COL["w_rz"]], rdot_tracking_gain=th[cg.COL["w_rd"]],
        w_tracking_gain=th[cg.COL["w_w"]], rel_pos_gain=th[cg.COL["w_rel"]], min_f_gain=th[cg.COL["w_f"]] / fs**2,
        force_switch_weight=th[cg.COL["w_sw"]] / fs**2, min_qddot_gain=th[cg.COL["gq"]], zmp_tracking_gain=th[cg.COL["w_zmp"]],
        lip_height=cg.G / th[cg.COL["eta2"]], friction_cone_coefficient=th[cg.COL["mu_lin"]] * np.sqrt(2.0),
        friction_barrier_weight=th[cg.COL["bar_w"]], friction_barrier_sharpness=th[cg.COL["bar_s"]], bound_barrier_weight=th[cg.COL["box_w"]],
        bound_barrier_sharpness=th[cg.COL["box_s"]], **({"feet8": feet} if model == "srbd61" else {"feet": feet}))


def _point(name, seed):
    _, x, u, P = pg.random_plan(name, 2, 1, seed)
    return x[0, 1], u[0, 1], P[0, 1]


def _check_against_the_oracle(name, cst, label, columns=None):
    J = cg.gradients(name, cst)
    th0 = cg.derived(cg.library_consts(name, cst))
    N, worst = 4, 0.0
    for seed, k in ((0, 0), (1, 2), (2, N)):                                    # node classes '0', 'k', 'N'
        x, u, p = _point(name, seed)
        terminal = k == N
        uu = np.zeros(J["nu"]) if terminal else u

        def both(th):
            f, _, _, _, L = cport.eval_knot(consts_of_derived(name, cst, th), x, uu, p, k, terminal, name)
            return np.array(f, dtype=float), L

        f0, L0 = both(th0)
        key = pg.node_class(k, N)
        assert abs(cg.cost(J, key, x, None if terminal else u, p, th0) - L0) <= E * EPS * max(1.0, abs(L0)), (label, k)
        g = cg.dL_dtheta(J, key, x, None if terminal else u, p, th0)
        F = cg.df_dtheta(J, x, uu, p, th0)
        if not terminal:
            assert np.max(np.abs(np.asarray(J["f"](x, u, p, th0[:31]), dtype=float).reshape(-1) - f0)) <= E * EPS * max(1.0, np.max(np.abs(f0)))
        for c in (range(31) if columns is None else columns):
            if cg.NAMES[c] == "w_rxy":
                continue                                                       # moves with w_rz
            if (cg.NAMES[c] in cg.FRICTION_COLS and not cst.friction_barrier_weight > 0.0) or \
                    (cg.NAMES[c] in cg.BOUND_COLS and not cst.bound_barrier_weight > 0.0):
                continue                                                       # a barrier that is off: a weight off 0 is another build
            pair = [c, cg.COL["w_rxy"]] if cg.NAMES[c] == "w_rz" else [c]
            h = 1e-3 * abs(th0[c]) if th0[c] != 0.0 else 1e-3
            e = np.zeros(32); e[pair] = 1.0

            def quotient(step):
                (fp, Lp), (fm, Lm) = both(th0 + step * e), both(th0 - step * e)
                return (fp - fm) / (2.0 * step), (Lp - Lm) / (2.0 * step)

            (dF1, dL1), (dF2, dL2) = quotient(h), quotient(2.0 * h)
            ref = float(np.sum(g[pair]))
            tol = 2.0 * abs(dL2 - dL1) / 3.0 + E * EPS * abs(L0) / h + E * EPS * (abs(ref) + 1.0)
            err = abs(dL1 - ref)
            assert err <= tol, f"{label} node {k} dL/d{cg.NAMES[c]}: {dL1} against {ref}, tolerance {tol:.3e} at h = {h:.3e}"
            worst = max(worst, err / tol)
            if not terminal:
                refF = F[:, pair].sum(axis=1)
                tolF = 2.0 * np.max(np.abs(dF2 - dF1)) / 3.0 + E * EPS * max(1.0, np.max(np.abs(f0))) / h + E * EPS * (np.max(np.abs(refF)) + 1.0)
                errF = np.max(np.abs(dF1 - refF))
                assert errF <= tolF, f"{label} node {k} df/d{cg.NAMES[c]}: off by {errF:.3e}, tolerance {tolF:.3e}"
                worst = max(worst, errF / tolF)
        # the columns the model does not read are structural zeros of the reference
        dead = cg.zero_columns(name, cst.friction_barrier_weight > 0.0, cst.bound_barrier_weight > 0.0)
        assert not np.any(g[dead]) and not np.any(F[:, dead]), label
    print(f"{label}: worst central-difference error / tolerance {worst:.3f}")
    return worst


@pytest.mark.parametrize("key", SETS)
@pytest.mark.parametrize("name", cg.MODELS)
def test_reference_against_central_differences_of_the_c_oracle(name, key):
    cst = kc.oracle_consts(name, _consts(name, key))
    _check_against_the_oracle(name, cst, f"{name} {key}")
    J = cg.gradients(name, cst)
    x, u, p = _point(name, 0)
    F = cg.df_dtheta(J, x, u, p, cg.derived(cg.library_consts(name, cst)))
    rows = {c: sorted(set(np.nonzero(F[:, c])[0])) for c in range(32) if np.any(F[:, c])}
    nx = J["nx"]
    if name == "lip30":
        assert set(rows) == {cg.COL["dt"], cg.COL["eta2"]} and rows[cg.COL["eta2"]] == [15, 16, 17]
    else:
        rd = 7 + (0 if name == "srbd13" else 12 if name == "srbd37" else 24)
        assert set(rows) == {0, 1, *range(2, 11)} and rows[1] == [rd, rd + 1, rd + 2]
        assert all(rows[c] == [rd + 3, rd + 4, rd + 5] for c in range(2, 11))
    assert len(rows[cg.COL["dt"]]) >= nx - 4                                     # dt enters every Euler row (a zero velocity aside)


@pytest.mark.parametrize("kind", ("bar", "box"))
def test_the_barrier_columns_against_the_c_oracle(kind):
    from tests import plan_audit_cases as pac
    consts = pac.problem("srbd13", 4, 1, kind)[2]
    cst = kc.oracle_consts("srbd13", consts)
    assert (cst.friction_barrier_weight > 0.0) == (kind == "bar") and (cst.bound_barrier_weight > 0.0) == (kind == "box")
    cols = [cg.COL[n] for n in (cg.FRICTION_COLS if kind == "bar" else cg.BOUND_COLS)]
    _check_against_the_oracle("srbd13", cst, f"srbd13 {kind}", columns=cols + [0, 1, 2, cg.COL["gq"]])


def test_envelope_experiment_on_the_c_oracle():
    """The envelope experiment of const_gradient_cases (srbd13, N = 8, the four robots and tight options of the parameter sensitivities'
    experiment, a direction over m, I, dt, rdot_tracking_gain and min_f_gain) with the C oracle's solves, the symbolic reference and the
    chain rule to the fields: all three solves of all four robots converge with closed gaps at every step (asserted inside), the
    figure falls as h^2 while truncation leads, and its smallest value over the scan and the h it is found at are the recorded
    ENVELOPE_DISCREPANCY and ENVELOPE_H (a rounding-level floor: to a factor of 2 on another CPU)."""
    scan = {h: d.max() for h, d in cg.envelope_scan().items()}
    for h, d in scan.items():
        print(f"h = {h:.0e}: discrepancy {d:.3e}")
    assert all(np.isfinite(d) for d in scan.values()) and len(scan) == len(cg.ENVELOPE_STEPS)
    assert 50.0 < scan[1e-2] / scan[1e-3] < 200.0                               # second order in h: C is the derivative, not near it
    best = min(scan, key=scan.get)
    assert 0.5 * cg.ENVELOPE_DISCREPANCY <= scan[best] <= 2.0 * cg.ENVELOPE_DISCREPANCY
    assert scan[cg.ENVELOPE_H] <= 2.0 * cg.ENVELOPE_DISCREPANCY and scan[cg.ENVELOPE_H] <= 1.3 * scan[best]


# ---- DDPSolver.constant_gradient on a stub engine ------------------------------------------------------------------------------------------
class _StubEngine:
    def __init__(self):
        self.calls = 0

    def const_gradient(self, first, count):
        self.calls += 1
        assert (first, count) == (0, 1)
        return np.arange(40.0)[None], [dict(m=-1.5, dt=2.0)]


def _solver(user=None, solved=True):
    from srbd_horizon_amd.ddp import DDPSolver
    s = DDPSolver.__new__(DDPSolver)
    s.ddp_solver, s._user, s.var_solution = _StubEngine(), user, ({} if solved else None)
    return s


def test_constant_gradient_of_the_solver_facade(lib):
    s = _solver()
    assert s.constant_gradient() == dict(m=-1.5, dt=2.0) and s.ddp_solver.calls == 1
    rec = s.constant_gradient_record
    assert list(rec) == list(cg.NAMES) + list(_lib.CONST_GRADIENT_TAIL) and len(rec) == 40
    assert rec["dt"] == 0.0 and rec["Is[8]"] == 10.0 and rec["box_s"] == 30.0 and rec["relative"] == 32.0 and rec["nodes"] == 37.0
    s = _solver(solved=False)
    with pytest.raises(RuntimeError, match="no solve has run"):
        s.constant_gradient()
    s = _solver(user=object())
    with pytest.raises(NotImplementedError, match="non-linear residuals"):
        s.constant_gradient()
    assert s.ddp_solver.calls == 0
