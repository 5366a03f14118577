"""What the constant-sensitivity tests share (tests/test_const_gradient_cpu.py, tests/test_gpu_const_gradient.py): the result of
sddp_const_gradient_range_device (include/sddp.h) stated once in numpy over SYMBOLIC derivatives in the derived constants, the
comparison of a device result with it, the chain rule to the fields of sddp_model_consts, and the cases.

THE GRADIENT of one instance, from a trajectory x [N + 1, nx], u [N, nu], the parameters P [N + 1, np], costates lam [N + 1, nx] and the
derived constants theta [32] (make_dev_consts of csrc/sddp_models.hpp, restated in derived()):
    node k < N:  A_k[c] = dL_k/dtheta_c + sum_i lam_{k+1}[i] df_k[i]/dtheta_c,      A_N[c] = dL_N/dtheta_c,      C[c] = sum_k A_k[c] in node order,
entry c of A_k starting at dL/dtheta_c and adding df[i]/dtheta_c lam_{k+1}[i] for i = 0 .. nx - 1 in this order.
THE RECORD (40 doubles): 0 .. 31 C; 32 max_c |C[c] theta_c|, 33 its column (-1 where word 32 is NaN); 34 - 36 words 4, 0, 6 of the
stationarity record; 37 N; 38, 39 zero.

Where the symbols come from.  tests/sym_models.py assemble(), the one statement of every model's layout, takes a constants object and
reads its fields; here it is handed one whose fields are sympy SYMBOLS arranged so that what it derives from them are the derived
constants themselves (force_scaling = 1, m = 1 / inv_ms, I = Is, min_f_gain = w_f, feet = the offsets, ...; w_rz, w_rxy and eta2 as
fields of their own, where a robot has one r_tracking_gain and a lip_height).  The two barriers are no residual rows of sym_models:
they are oracle/models.py's formulas (_force_rows, friction_cone_rows, _bound_rows), present where the weight is > 0 as there.  One
block is not sym_models': _srbd takes symbols for the inertia, but with them its adjugate / determinant of R(o) Is R(o)^T takes minutes
per model (inertia_mode 1); the accelerations are written here from oracle/models.py srbd_acc's formulas with the rotation matrix as
nine PLACEHOLDER symbols, filled with quat_to_rot(o) when a function is called, and handed to assemble() as its dynamics hook: R does
not depend on a constant, so the derivative in theta at fixed R is the derivative.  The cost is the sum of the squared
rows, so sqrt(gain)^2 = gain and no square root of a constant is left to differentiate.  What selects code has no symbol: inertia_mode,
lever_sign, relative_velocity_constraints, the bounds; an expression set is cached per such selection, whatever the numbers.
"""
import functools
import types

import numpy as np
import sympy as sp

from oracle import models as omodels
from srbd_horizon_amd import _lib
from tests import param_gradient_cases as pg, sym_models as sm
from tests.param_gradient_cases import _arr, node_class

W, COLS = _lib.CONST_GRADIENT_WORDS, _lib.CONST_GRADIENT_COLS
REL, COLUMN, LAM0, STAT, DEFECT, NODES = range(COLS, COLS + 6)
MODELS = ("srbd13", "srbd37", "lip30", "srbd61")
RTOL = 1e-11      # the inspectors' tolerance (tests/param_gradient_cases.py RTOL), here of a column's magnitude sum
G = 9.81

NAMES = ("dt", "inv_ms", *(f"Is[{i}]" for i in range(9)), "com_z", "w_rz", "w_rxy", "w_rd", "w_w", "w_rel", "w_f", "w_sw", "gq", "w_zmp", "eta2",
         "d1x", "d1y", "d2x", "d2y", "mu_lin", "bar_w", "bar_s", "box_w", "box_s", "reserved")
COL = {n: i for i, n in enumerate(NAMES)}
TH = sp.symbols("th0:%d" % (COLS - 1))            # the 31 live columns; column 31 is reserved
FIELD_NAMES = ("m", *(f"I[{i}]" for i in range(9)), *(f"com[{i}]" for i in range(3)), *(f"feet[{i}]" for i in range(12)), "dt", "force_scaling",
               "r_tracking_gain", "rdot_tracking_gain", "w_tracking_gain", "rel_pos_gain", "force_switch_weight", "min_qddot_gain", "min_f_gain",
               "zmp_tracking_gain", "lip_height", "friction_cone_coefficient", "friction_barrier_weight", "friction_barrier_sharpness",
               "bound_barrier_weight", "bound_barrier_sharpness")
# which columns a model reads at all (the others are exact zeros on the device)
_SRBD_COLS = ("dt", "inv_ms", *(f"Is[{i}]" for i in range(9)), "com_z", "w_rz", "w_rd", "w_w", "w_f", "w_sw", "gq")
_FEET_COLS = ("w_rel", "d1x", "d1y", "d2x", "d2y")
READS = {"srbd13": _SRBD_COLS, "srbd37": _SRBD_COLS + _FEET_COLS, "srbd61": _SRBD_COLS + _FEET_COLS,
         "lip30": ("dt", "com_z", "w_rz", "w_rxy", "w_rd", "gq", "w_zmp", "eta2") + _FEET_COLS}
FRICTION_COLS, BOUND_COLS = ("mu_lin", "bar_w", "bar_s"), ("box_w", "box_s")


# ---- the constants: fields -> derived (make_dev_consts restated), and the chain rule back ---------------------------------------------------
def flat_fields(consts):
    """a constants dict of the library (or a RobotConsts; feet = the library's four contact points) -> the 41 field values in the order
    of FIELD_NAMES"""
    base_consts = omodels.RobotConsts()      # (a dict may leave out what it keeps at the default: the barrier constants)
    get = (lambda k: consts.get(k, getattr(base_consts, k))) if isinstance(consts, dict) else (lambda k: getattr(consts, k))
    out = []
    for name in FIELD_NAMES:
        base, _, idx = name.partition("[")
        v = get(base)
        out.append(float(np.asarray(v, dtype=float).reshape(-1)[int(idx[:-1])]) if idx else float(v))
    return np.array(out)


def derived_of_fields(v):
    """make_dev_consts on the 41 field values -> theta [32]"""
    f = dict(zip(FIELD_NAMES, v))
    fs = f["force_scaling"]
    th = np.zeros(COLS)
    th[COL["dt"]], th[COL["inv_ms"]] = f["dt"], fs / f["m"]
    for i in range(9):
        th[2 + i] = f[f"I[{i}]"] / fs
    th[COL["com_z"]] = f["com[2]"]
    th[COL["w_rz"]] = th[COL["w_rxy"]] = f["r_tracking_gain"]
    th[COL["w_rd"]], th[COL["w_w"]], th[COL["w_rel"]] = f["rdot_tracking_gain"], f["w_tracking_gain"], f["rel_pos_gain"]
    th[COL["w_f"]], th[COL["w_sw"]] = fs * fs * f["min_f_gain"], fs * fs * f["force_switch_weight"]
    th[COL["gq"]], th[COL["w_zmp"]], th[COL["eta2"]] = f["min_qddot_gain"], f["zmp_tracking_gain"], G / f["lip_height"]
    th[COL["d1x"]], th[COL["d1y"]] = f["feet[6]"] - f["feet[0]"], f["feet[7]"] - f["feet[1]"]
    th[COL["d2x"]], th[COL["d2y"]] = f["feet[9]"] - f["feet[3]"], f["feet[10]"] - f["feet[4]"]
    th[COL["mu_lin"]] = f["friction_cone_coefficient"] / np.sqrt(2.0)
    th[COL["bar_w"]], th[COL["bar_s"]] = f["friction_barrier_weight"], f["friction_barrier_sharpness"]
    th[COL["box_w"]], th[COL["box_s"]] = f["bound_barrier_weight"], f["bound_barrier_sharpness"]
    return th


def derived(consts):
    return derived_of_fields(flat_fields(consts))


def library_consts(model, cst):
    """a RobotConsts -> what flat_fields reads: srbd61's four library contact points are feet8[:4] (tests/consts_cases.py)"""
    d = {k: getattr(cst, k) for k in set(n.partition("[")[0] for n in FIELD_NAMES)}
    if model == "srbd61":
        d["feet"] = np.asarray(cst.feet8, dtype=float)[:4]
    return d


# ---- the symbolic reference ------------------------------------------------------------------------------------------------------------------
def _sym_consts(inertia_mode, lever_sign, rel_vel):
    t = dict(zip(NAMES, TH))
    feet = np.array([[0, 0, 0], [0, 0, 0], [t["d1x"], t["d1y"], 0], [t["d2x"], t["d2y"], 0]], dtype=object)
    return types.SimpleNamespace(
        force_scaling=sp.Integer(1), m=1 / t["inv_ms"], I=np.array([t[f"Is[{i}]"] for i in range(9)], dtype=object).reshape(3, 3),
        inertia_mode=inertia_mode, lever_sign=lever_sign, relative_velocity_constraints=rel_vel, com=(0, 0, t["com_z"]),
        r_tracking_gain=t["w_rz"], rdot_tracking_gain=t["w_rd"], w_tracking_gain=t["w_w"], rel_pos_gain=t["w_rel"], min_f_gain=t["w_f"],
        force_switch_weight=t["w_sw"], min_qddot_gain=t["gq"], feet=feet, feet8=np.vstack([feet, feet]), dt=t["dt"],
        zmp_tracking_gain=t["w_zmp"], w_rz=t["w_rz"], w_rxy=t["w_rxy"], eta2=t["eta2"]), t


RS = sp.symbols("R0:9")                         # the rotation matrix of the state's quaternion, row-major: placeholders (see above)


def _srbd(t, cst, r, o, w, cs, fs):
    """rddot, wdot of oracle/models.py srbd_acc / world_inertia in the derived constants: rddot = inv_ms sum f - g e_z,
    I_w wdot = s sum (c_i - r) x f_i - w x I_w w, I_w = R o Is o R^T element-wise (inertia_mode 0) or R Is R^T (1); and odot"""
    R = sp.Matrix(3, 3, RS)
    Is = sp.Matrix(3, 3, [t[f"Is[{i}]"] for i in range(9)])
    M = sp.Matrix(3, 3, lambda i, j: R[i, j] * Is[i, j] * R[j, i]) if cst.inertia_mode == 0 else R * Is * R.T
    rddot = sp.Matrix([0, 0, -sm.G])
    tau = sp.zeros(3, 1)
    for c, f in zip(cs, fs):
        rddot += t["inv_ms"] * f
        tau += cst.lever_sign * (c - r).cross(f)
    tau -= w.cross(M * w)
    return rddot, (M.adjugate() / M.det()) * tau, sp.Rational(1, 2) * sm._qmul(sp.Matrix([w[0], w[1], w[2], 0]), o)


def _sq(rows):
    return sum((sp.Mul(r, r) for r in rows), sp.Integer(0))


def assemble(name, inertia_mode=0, lever_sign=1.0, rel_vel=True, friction=False, bounds=None):
    """(x, u, p, f, Li, Ls): the symbols, the model step and the cost of the input and of the state class in TH.  friction: the
    friction-cone barrier is on; bounds: (lower, upper) of the bound barrier, or None where it is off"""
    cst, t = _sym_consts(inertia_mode, lever_sign, rel_vel)
    x, u, p, f, ires, sres, fs = sm.assemble(name, cst, srbd=functools.partial(_srbd, t))
    nx, nu = len(x), len(u)
    Li, Ls = _sq(ires), _sq(sres)
    if friction:      # oracle/models.py _force_rows: w sum_j exp(s a_j . f), a_j the rows of friction_cone_rows with mu / sqrt(2) = mu_lin
        ml = t["mu_lin"]
        A = sp.Matrix([[1, 0, -ml], [-1, 0, -ml], [0, 1, -ml], [0, -1, -ml], [0, 0, -1]])
        for f_i in fs:
            Li += t["bar_w"] * sum(sp.exp(t["bar_s"] * a) for a in A * f_i)
    if bounds is not None:      # oracle/models.py _bound_rows
        lb, ub = (np.asarray(b, dtype=float)[:nx + nu] for b in bounds)
        zz = [*x, *u]
        for j in range(nx + nu):
            if np.isfinite(ub[j]):
                Li += t["box_w"] * sp.exp(t["box_s"] * (zz[j] - float(ub[j])))
            if np.isfinite(lb[j]):
                Li += t["box_w"] * sp.exp(t["box_s"] * (float(lb[j]) - zz[j]))
    assert not any(q.exp == sp.Rational(1, 2) for e in (Li, Ls) for q in e.atoms(sp.Pow)), "a square root of a constant is left"
    return x, u, p, f, Li, Ls


def _bounds_key(bounds):
    return None if bounds is None else tuple(np.asarray(b, dtype=float).tobytes() for b in bounds)


@functools.lru_cache(maxsize=None)
def _gradients(name, inertia_mode, lever_sign, rel_vel, friction, bkey):
    bounds = None if bkey is None else tuple(np.frombuffer(b) for b in bkey)
    x, u, p, f, Li, Ls = assemble(name, inertia_mode, lever_sign, rel_vel, friction, bounds)
    args = (list(x), list(u), list(p), list(TH), list(RS))
    quat = None if name == "lip30" else slice(3, 7)

    def lam(e):
        fn = sp.lambdify(args, e, "numpy", cse=True)
        return lambda xv, uv, pv, tv: fn(xv, uv, pv, tv, np.zeros(9) if quat is None else omodels.quat_to_rot(np.asarray(xv, dtype=float)[quat]).reshape(-1))

    th = sp.Matrix(TH)
    return dict(f=lam(f), Li=lam(Li), Ls=lam(Ls), dLi=lam(sp.Matrix([Li]).jacobian(th)), dLs=lam(sp.Matrix([Ls]).jacobian(th)),
                Fth=lam(f.jacobian(th)), nx=len(x), nu=len(u), np=len(p))


def gradients(name, cst):
    """the compiled cost, step and their SYMBOLIC derivatives in TH for the code selection of the RobotConsts cst: functions of
    (x, u, p, theta[:31]): "f" [nx], "Li", "Ls", "dLi" [31], "dLs" [31], "Fth" [nx, 31]; cached per selection"""
    bounds = (cst.lower, cst.upper) if cst.bound_barrier_weight > 0.0 else None
    return _gradients(name, int(cst.inertia_mode), float(cst.lever_sign), bool(cst.relative_velocity_constraints),
                      bool(cst.friction_barrier_weight > 0.0), _bounds_key(bounds))


def cost(J, key, x, u, p, th):
    u = np.zeros(J["nu"]) if u is None else u
    p, t = p[:J["np"]], th[:COLS - 1]
    return (0.0 if key == "N" else float(J["Li"](x, u, p, t))) + (0.0 if key == "0" else float(J["Ls"](x, u, p, t)))


def dL_dtheta(J, key, x, u, p, th):
    """dL/dtheta [32] of node class key in {'0', 'k', 'N'}"""
    u = np.zeros(J["nu"]) if u is None else u
    p, t = p[:J["np"]], th[:COLS - 1]
    g = np.zeros(COLS)
    if key != "N":
        g[:COLS - 1] += _arr(J["dLi"](x, u, p, t), (1, COLS - 1))[0]
    if key != "0":
        g[:COLS - 1] += _arr(J["dLs"](x, u, p, t), (1, COLS - 1))[0]
    return g


def df_dtheta(J, x, u, p, th):
    F = np.zeros((J["nx"], COLS))
    F[:, :COLS - 1] = _arr(J["Fth"](x, u, p[:J["np"]], th[:COLS - 1]), (J["nx"], COLS - 1))
    return F


def node_addends(J, k, N, x, u, p, lam_next, th):
    """(A_k [32], magnitudes [32]) of node k"""
    g = dL_dtheta(J, node_class(k, N), x, u, p, th)
    m = np.abs(g)
    if k < N:
        F = df_dtheta(J, x, u, p, th)
        for i in range(J["nx"]):
            g = g + F[i] * lam_next[i]
            m = m + np.abs(F[i]) * abs(lam_next[i])
    return g, m


def in_order_sum(nodes):
    """[N + 1, 32] -> the columns added in node order, starting at 0.0 (what the device's summing lanes do)"""
    acc = np.zeros(nodes.shape[1])
    for row in nodes:
        acc = acc + row
    return acc


def tail_of(C, th):
    """words 32, 33 of a record from its columns"""
    with np.errstate(invalid="ignore", over="ignore"):
        rel = np.abs(C * th)
    if np.isnan(rel).any():
        return np.nan, -1.0
    best = 0
    for j in range(COLS):
        if rel[j] > rel[best]:
            best = j
    return rel[best], float(best)


def reference(J, th, x, u, P, lam):
    """-> (nodes [N + 1, 32], C [32], magnitude sums [32]) of one instance, with the costates lam [N + 1, nx] given"""
    x, u, P, lam = (np.asarray(a, dtype=float) for a in (x, u, P, lam))
    N = u.shape[0]
    A, M = np.zeros((N + 1, COLS)), np.zeros((N + 1, COLS))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(N + 1):
            A[k], M[k] = node_addends(J, k, N, x[k], u[k] if k < N else None, P[k], lam[k + 1] if k < N else None, th)
    return A, in_order_sum(A), M.sum(axis=0)


def assert_result(rec, nodes, ref, th, label=""):
    """a device record and its addends against reference(): every column, and every addend, within RTOL x the column's magnitude sum;
    what a record promises of itself exactly -> worst error / tolerance"""
    Ar, Cr, Mr = ref
    tol = RTOL * Mr
    err_c, err_n = np.abs(rec[:COLS] - Cr), np.max(np.abs(nodes - Ar), axis=0)
    for j in range(COLS):
        assert err_c[j] <= tol[j] and err_n[j] <= tol[j], \
            f"{label}: column {NAMES[j]} off by {err_c[j]:.3e} (addends {err_n[j]:.3e}), tolerance {tol[j]:.3e}; {rec[j]} against {Cr[j]}"
    assert_exact(rec, nodes, th, label)
    live = tol > 0.0
    return float(np.max(np.maximum(err_c, err_n)[live] / tol[live], initial=0.0))


def assert_exact(rec, nodes, th, label=""):
    """the record is the in-order sum of its own rows, bit for bit; words 32, 33 follow from the columns; 37 .. 39"""
    assert rec[:COLS].tobytes() == in_order_sum(nodes).tobytes(), f"{label}: the columns are not the in-order sums of the addends"
    top, at = tail_of(rec[:COLS], th)
    assert (np.isnan(rec[REL]) and np.isnan(top)) or rec[REL] == top, f"{label}: word 32 {rec[REL]} against {top}"
    assert rec[COLUMN] == at, f"{label}: word 33 {rec[COLUMN]} against {at}"
    assert rec[NODES] == nodes.shape[0] - 1 and rec[COLS - 1] == 0.0 and np.all(rec[W - 2:] == 0.0), label
    assert np.all(nodes[:, COLS - 1] == 0.0), label


def zero_columns(model, friction=False, box=False):
    """the columns that are exact zeros on the device for a model and build"""
    live = set(READS[model]) | (set(FRICTION_COLS) if friction else set()) | (set(BOUND_COLS) if box else set())
    return [COL[n] for n in NAMES if n not in live]


# ---- the envelope experiment with theta in place of P ----------------------------------------------------------------------------------------
# srbd13, N = 8, the four robots and the tight options of tests/param_gradient_cases.py.  The direction runs over the FIELDS m, I, dt,
# rdot_tracking_gain and min_f_gain, each moved by a fixed fraction of its value (another per field, I by a symmetric push);
# J*(theta +- h delta) is the cost the solver converges to from the base optimum.  The discrepancy of an instance is
#     | sum_f D[f] delta[f]  -  (J*(+h) - J*(-h)) / 2h |  /  sum_f |D[f] delta[f]|,      D = the chain rule of C to the fields,
# its figure the maximum over the four.
# ENVELOPE_H and ENVELOPE_DISCREPANCY are what envelope_scan() measures on the CPU with the C oracle's solves and the symbolic reference
# (tests/test_const_gradient_cpu.py asserts them again; they are recorded in profiles/const_gradient/README.md): the h of the scan with
# the smallest figure, and that figure.  The GPU test uses this h and allows 10 x the figure, the margin the parameter sensitivities
# took, for the same reason: the figure rests on the base solve's own distance from stationarity.
ENVELOPE_STEPS = (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6)
# measured: the figure falls as h^2 from 6.6e-4 at h = 1e-1 to 5.4e-9 at 3e-4 and then stays between 2.4e-9 and 3.1e-9 down to h = 1e-6
ENVELOPE_H = 1e-4
ENVELOPE_DISCREPANCY = 2.35e-9


def envelope_direction(consts):
    """the 41-vector delta (in the order of FIELD_NAMES) for a constants dict"""
    v = flat_fields(consts)
    d = np.zeros(len(FIELD_NAMES))
    idx = {n: i for i, n in enumerate(FIELD_NAMES)}
    d[idx["m"]] = 0.5 * v[idx["m"]]
    push = np.array([[0.4, 0.05, -0.03], [0.05, -0.3, 0.02], [-0.03, 0.02, 0.5]]) * np.sqrt(np.outer(*(2 * [np.diag(v[1:10].reshape(3, 3))])))
    d[1:10] = push.reshape(-1)
    d[idx["dt"]] = -0.3 * v[idx["dt"]]
    d[idx["rdot_tracking_gain"]] = 0.6 * v[idx["rdot_tracking_gain"]]
    d[idx["min_f_gain"]] = -0.7 * v[idx["min_f_gain"]]
    return d


def moved_consts(consts, delta, h):
    """the constants dict with every field of the direction at value + h delta"""
    v = dict(zip(FIELD_NAMES, flat_fields(consts) + h * delta))
    out = dict(consts)
    out.update(m=v["m"], I=np.array([v[f"I[{i}]"] for i in range(9)]).reshape(3, 3), dt=v["dt"], rdot_tracking_gain=v["rdot_tracking_gain"],
               min_f_gain=v["min_f_gain"])
    return out


def fields_of(consts, C):
    """the chain rule from a derived gradient C [32] to the 41 fields, NUMERICALLY: field i moves by +-h, h = 1e-6 max(1, |value|), and
    D[i] = C . (derived(v + h e_i) - derived(v - h e_i)) / 2h -> (D [41], magnitudes [41] = |C| . |that difference quotient|).
    Every entry of theta is a polynomial of degree <= 2 or a reciprocal in one field, so the quotient's truncation error is below
    1e-12 of it and its rounding about eps / 1e-6 = 2e-10 of it: FIELDS_RTOL of the magnitude covers both with a margin of 50."""
    v = flat_fields(consts)
    out, mag = np.zeros(len(v)), np.zeros(len(v))
    for i in range(len(v)):
        h = 1e-6 * max(1.0, abs(v[i]))
        e = np.zeros(len(v)); e[i] = h
        q = (derived_of_fields(v + e) - derived_of_fields(v - e)) / (2.0 * h)
        out[i], mag[i] = C @ q, np.abs(C) @ np.abs(q)
    return out, mag


FIELDS_RTOL = 1e-8


def envelope_discrepancy(D, delta, Jp, Jm, h):
    """the figure of every instance: D [B, 41] the gradients in the fields, the costs J*(+h), J*(-h) [B] -> [B]"""
    return pg.central_discrepancy(D @ delta, np.sum(np.abs(D * delta[None]), axis=1), Jp, Jm, h)


def envelope_problem():
    """-> (batch, delta [41]): the start of tests/param_gradient_cases.py's experiment and the direction in the fields"""
    batch = pg.envelope_problem()[0]
    return batch, envelope_direction(batch["consts"])


def envelope_scan(steps=ENVELOPE_STEPS):
    """the experiment on the CPU with the C oracle's solves and the symbolic reference -> {h: the figure [B]}; asserts that all three
    solves of every instance converge with closed gaps"""
    from tests import stationarity_cases as sc
    batch, delta = envelope_problem()
    cst = omodels.RobotConsts(**batch["consts"])
    x, u, _ = pg.converged_solve(batch, batch["xs"], batch["us"], cst=cst)
    J, th, m = gradients(pg.ENVELOPE_MODEL, cst), derived(batch["consts"]), omodels.make_model(pg.ENVELOPE_MODEL, cst)
    D = np.stack([fields_of(batch["consts"], reference(J, th, x[b], u[b], batch["params"][b],
                                                       sc.model_reference(m, x[b], u[b], batch["params"][b])[1])[1])[0]
                  for b in range(x.shape[0])])
    out = {}
    for h in steps:
        Jp, Jm = (pg.converged_solve(batch, x, u, cst=omodels.RobotConsts(**moved_consts(batch["consts"], delta, s * h)))[2] for s in (1.0, -1.0))
        out[h] = envelope_discrepancy(D, delta, Jp, Jm, h)
    return out


def flat_of_field_dict(fields):
    """a dict by sddp_model_consts field name (DdpEngine.const_gradient_fields) -> the 41 values in the order of FIELD_NAMES"""
    return flat_fields(fields)
