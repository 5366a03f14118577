"""The model constants away from their defaults: the case table that tests/test_consts_cases_cpu.py (would a dropped, swapped or
mis-derived constant show? -- numpy and C oracle only) and tests/test_gpu_consts.py (every kernel family against the oracle) share.
No GPU needed.

sddp_model_consts is the whole description of the robot a caller hands to the library; make_dev_consts (csrc/sddp_models.hpp) folds
it into the record every kernel reads.  The other GPU tests run on almost one robot, the workload's, whose constants are the defaults.

FIELDS    every field of sddp_model_consts that is not a build selector (the barrier weights and sharpnesses, the bounds and extra_*
          are out), each with ONE off-default value.  Scalars move by a fixed factor inside [0.5, 2] (the range of
          variant_cases.draw), another factor for every field, so two fields that a kernel swapped cannot cancel; I becomes a
          symmetric positive-definite matrix that is no multiple of the default; com moves in all three components; feet move by
          another offset per contact point (d1 != d2, left differs from right); inertia_mode 1, lever_sign -1,
          relative_velocity_constraints 0; friction_cone_coefficient 0.5, which only matters with the friction barrier on: its
          case runs on the "bar" build (BAR).
APPLIES   model -> the fields that move that model's f, F, g, H or L at all, as a literal table.  What is NOT listed is inert in the
          oracle; test_consts_cases_cpu.py checks both directions, component by component for com and feet (COMPONENTS: only com z
          and the x / y of the feet are read by the problem's graphs; com x / y and the feet's z only enter the initial state and
          the c_ref parameters, which the caller builds).
ALL_OFF   model -> the constants with every applicable field off-default at once (a dict for DdpEngine / eval_knots; oracle_consts
          makes the oracle's RobotConsts of it).
draw_all  every field of _lib.INSTANCE_CONST_FIELDS drawn per instance from one seeded generator; the integer fields and lever_sign
          take both of their values within the batch.

srbd61: the library's `feet` are contact points 0..3 of the eight-point model, the oracle's RobotConsts.feet8[:4] (oracle_consts).
"""
import dataclasses

import numpy as np

from oracle import models as omodels
from tests import oracle_refs as refs

MODELS = ("srbd13", "srbd37", "lip30", "srbd61")

SCALE = dict(m=1.3, dt=0.8, force_scaling=0.7, r_tracking_gain=1.7, rdot_tracking_gain=0.6, w_tracking_gain=1.45, rel_pos_gain=0.55,
             force_switch_weight=1.9, min_qddot_gain=1.6, min_f_gain=0.65, zmp_tracking_gain=1.25, lip_height=0.85)
GAINS = ("r_tracking_gain", "rdot_tracking_gain", "w_tracking_gain", "rel_pos_gain", "force_switch_weight", "min_qddot_gain", "min_f_gain",
         "zmp_tracking_gain")      # the same-typed gain fields: any two of them exchanged must show
I_OFF = np.array([[2.6, -0.11, 0.07], [-0.11, 1.3, 0.09], [0.07, 0.09, 0.9]])
COM_OFF = np.array([0.03, -0.02, 0.93])
FEET_SHIFT = np.array([[0.01, 0.01, 0.01], [0.01, 0.02, -0.01], [0.005, 0.01, 0.02], [0.005, -0.005, 0.015]])
FIELDS = (*SCALE, "I", "com", "feet", "inertia_mode", "lever_sign", "relative_velocity_constraints", "friction_cone_coefficient")
FRICTION = dict(friction_barrier_weight=2.0, friction_barrier_sharpness=4.0)      # the barrier of tests/sweep_cases.py
BAR = ("friction_cone_coefficient",)                                              # fields whose case runs with FRICTION on

_SRBD = ("m", "I", "com", "dt", "force_scaling", "r_tracking_gain", "rdot_tracking_gain", "w_tracking_gain", "force_switch_weight",
         "min_qddot_gain", "min_f_gain", "inertia_mode", "lever_sign", "friction_cone_coefficient")
_CONTACT_STATES = ("feet", "rel_pos_gain", "relative_velocity_constraints")
APPLIES = {"srbd13": frozenset(_SRBD),
           "srbd37": frozenset(_SRBD + _CONTACT_STATES),
           "srbd61": frozenset(_SRBD + _CONTACT_STATES),
           "lip30": frozenset(("com", "dt", "r_tracking_gain", "rdot_tracking_gain", "min_qddot_gain", "zmp_tracking_gain", "lip_height")
                              + _CONTACT_STATES)}
# the components of com [3] and feet [4, 3] the graphs read (prb.py:184, :153-154): what DevConsts keeps (com_z, d1x, d1y, d2x, d2y)
COMPONENTS = {"com": np.array([False, False, True]), "feet": np.tile([True, True, False], (4, 1))}


def defaults(model):
    """the workload's constants of `model` (the library's defaults, written out): a fresh dict"""
    return {k: (np.array(v, dtype=float) if np.ndim(v) else v) for k, v in refs.batch(model, 1, [0])["consts"].items()}


def off_value(model, field, base=None):
    base = defaults(model) if base is None else base
    if field in SCALE:
        return base[field] * SCALE[field]
    return {"I": I_OFF.copy(), "com": COM_OFF.copy(), "feet": np.asarray(base["feet"], dtype=float).reshape(4, 3) + FEET_SHIFT,
            "inertia_mode": 1, "lever_sign": -1.0, "relative_velocity_constraints": 0, "friction_cone_coefficient": 0.5}[field]


def moved(model, fields, **more):
    """the defaults of `model` with `fields` at their off-default values (and FRICTION on where one of them needs it)"""
    c = defaults(model)
    for f in fields:
        c[f] = off_value(model, f, c)
    if any(f in BAR for f in fields):
        c.update(FRICTION)
    c.update(more)
    return c


def all_off(model, bar=False):
    """every applicable field of `model` off-default at once; friction_cone_coefficient only with `bar` (it selects nothing without
    the barrier, and with it the build is another)"""
    return moved(model, [f for f in FIELDS if f in APPLIES[model] and (bar or f not in BAR)])


ALL_OFF = {m: all_off(m) for m in MODELS}


def oracle_consts(model, consts):
    """oracle.models.RobotConsts of a constants dict of the library (extra keys such as extra_rows pass through)"""
    c = omodels.RobotConsts(**{k: v for k, v in consts.items()})
    if model == "srbd61":
        feet8 = np.array(omodels.RobotConsts().feet8, dtype=float)
        feet8[:4] = np.asarray(consts["feet"], dtype=float).reshape(4, 3)
        c = dataclasses.replace(c, feet8=feet8)
    return c


def oracle_model(model, consts):
    return omodels.make_model(model, oracle_consts(model, consts))


# ---- per-knot evaluation: the points of test_eval_knots_matches_oracle at N = 3 --------------------------------------------------------
KNOT_N = 3
KNOTS = np.array([0, 1, KNOT_N - 1, KNOT_N], dtype=np.int32)


def knot_points(model):
    """-> X [4, nx], U [4, nu], P [4, np]: the default robot's nominal point plus 0.05 N(0, 1), one per knot of KNOTS (the same points
    for every constants case of a model: the constants alone differ)"""
    m = omodels.make_model(model)
    rng = np.random.default_rng(5)
    nk = len(KNOTS)
    X = np.tile(m.initial_state(), (nk, 1)) + 0.05 * rng.standard_normal((nk, m.nx))
    U = np.tile(m.static_input(), (nk, 1)) + 0.05 * rng.standard_normal((nk, m.nu))
    P = np.tile(m.default_params(KNOT_N)[1], (nk, 1)) + 0.05 * rng.standard_normal((nk, m.np_))
    return X, U, P


def oracle_knots(model, consts, numpy=True):
    """-> f [4, nx], F [4, nx, nz], H [4, nz, nz], g [4, nz], L [4] of the numpy oracle (numpy=False: the C oracle) at knot_points, in
    eval_knots' layout: a terminal knot has f = F = 0 and only the state block of H and g"""
    from oracle import cport
    X, U, P = knot_points(model)
    cst = oracle_consts(model, consts)
    m = omodels.make_model(model, cst)
    nz = m.nx + m.nu
    f = np.zeros((len(KNOTS), m.nx)); F = np.zeros((len(KNOTS), m.nx, nz)); H = np.zeros((len(KNOTS), nz, nz))
    g = np.zeros((len(KNOTS), nz)); L = np.zeros(len(KNOTS))
    for t, k in enumerate(KNOTS):
        term = k == KNOT_N
        if not numpy:
            f[t], F[t], H[t], g[t], L[t] = cport.eval_knot(cst, X[t], U[t], P[t], int(k), term, model)
            if term:
                f[t] = 0.0; F[t] = 0.0
            continue
        if term:
            L[t], lx, _, lxx, _, _ = m.cost_derivs(X[t], None, P[t], int(k))
            H[t, :m.nx, :m.nx] = lxx; g[t, :m.nx] = lx
        else:
            f[t] = m.f(X[t], U[t], P[t])
            F[t] = np.hstack(m.f_jac(X[t], U[t], P[t]))
            L[t], lx, lu, lxx, lux, luu = m.cost_derivs(X[t], U[t], P[t], int(k))
            H[t] = np.block([[lxx, lux.T], [lux, luu]]); g[t] = np.concatenate([lx, lu])
    return f, F, H, g, L


def knot_excess(got, ref):
    """largest |got - ref| / tolerance over the stage knots' f and F and every knot's H, g, L, with the tolerances of
    test_eval_knots_matches_oracle: f rtol 1e-12 atol 1e-13; F rtol 1e-11 atol 1e-12; L 1e-12 max(1, |L|); g and H rtol 1e-11 with the
    floor 1e-11 max(1, max|.|) per knot.  <= 1 passes.  -> (worst, {name: excess})"""
    f, F, H, g, L = got
    fo, Fo, Ho, go, Lo = ref
    stage = KNOTS < KNOT_N
    floor = lambda a: np.maximum(1.0, np.max(np.abs(a.reshape(len(a), -1)), axis=1)).reshape((-1,) + (1,) * (a.ndim - 1))      # noqa: E731
    ex = dict(f=np.max(np.abs(f - fo)[stage] / (1e-12 * np.abs(fo) + 1e-13)[stage]),
              F=np.max(np.abs(F - Fo)[stage] / (1e-11 * np.abs(Fo) + 1e-12)[stage]),
              L=np.max(np.abs(L - Lo) / (1e-12 * np.maximum(1.0, np.abs(Lo)))),
              g=np.max(np.abs(g - go) / (1e-11 * np.abs(go) + 1e-11 * floor(go))),
              H=np.max(np.abs(H - Ho) / (1e-11 * np.abs(Ho) + 1e-11 * floor(Ho))))
    ex = {k: float(v) for k, v in ex.items()}
    return max(ex.values()), ex


# ---- one sweep, one rollout and whole solves with ALL_OFF ---------------------------------------------------------------------------------
BASE = refs.BASE
# (model, N, waves_per_simd builds): the smallest shapes tests/sweep_cases.py uses per family; theta = 1, mu = 1e-6, open gaps
SWEEPS = (("srbd13", 3, (1, 2)), ("srbd37", 2, (1,)), ("lip30", 2, (2,)), ("srbd61", 1, (1,)))
SO2_SWEEPS = (("srbd13", 3), ("srbd37", 2))      # the second_order = 2 builds: the same shapes, mode 2
SWEEP_SEEDS = {"srbd13": (2, 9), "srbd37": (3, 8), "srbd61": (1, 4), "lip30": (5, 0)}      # tests/sweep_cases.py SEEDS
SWEEP_CUT, SWEEP_NOISE, SWEEP_THETA, SWEEP_MU = 2, 1e-3, 1.0, 1e-6
SWEEP_ALPHAS = (1.0, 0.25)
# whole solves, B = 4: srbd13 and srbd37 at N = 6; lip30 and srbd61 at the smallest N of their whole-solve tests
# (tests/horizon_cases.py); the seeds are those on which the C oracle's two builds agree on the iteration count
# (tests/test_consts_cases_cpu.py)
SOLVES = {"srbd13": (6, (0, 1, 2, 3)), "srbd37": (6, (0, 1, 2, 3)), "lip30": (1, (0, 1, 2, 3)), "srbd61": (1, (0, 1, 2, 3))}
# lip30 is linear-quadratic and ends after one iteration under BASE: with alpha_0 = 0.5 (the a05 cases of tests/horizon_cases.py) the
# solve takes some 25 steps, each through lip_height and zmp_tracking_gain
SOLVE_OPTS = {"lip30": dict(alpha_0=0.5)}


def solve_options(model):
    return refs.options(SOLVE_OPTS.get(model, {}))


def problem(model, N, seeds, consts=None):
    """the workload's batch of `seeds` for the robot `consts` (default ALL_OFF): the start is the workload's (the default robot's
    stance), the constants the solver and the oracle get are `consts` -> dict(x0, params, xs, us, consts)"""
    return dict(refs.batch(model, N, seeds), consts=dict(ALL_OFF[model] if consts is None else consts))


def sweep_start(model, N, consts=None, mode=1):
    """as tests/sweep_cases.py _start / _trajectory: the numpy oracle's own solve under the case's constants (second_order = mode)
    cut at SWEEP_CUT iterations, plus SWEEP_NOISE x N(0, 1) on every state and input (x_0 stays) -> (problem, model, xs, us)"""
    from oracle import ddp as oddp
    s = problem(model, N, SWEEP_SEEDS[model], consts)
    m = oracle_model(model, s["consts"])
    opt = oddp.DdpOptions(**dict(BASE, max_iters=SWEEP_CUT, second_order=mode))
    res = [oddp.solve(m, s["x0"][b], s["params"][b], s["xs"][b], s["us"][b], opt) for b in range(len(s["x0"]))]
    xs, us = np.stack([r.xs for r in res]), np.stack([r.us for r in res])
    rng = np.random.default_rng(1)
    xs = xs + SWEEP_NOISE * rng.standard_normal(xs.shape)
    us = us + SWEEP_NOISE * rng.standard_normal(us.shape)
    xs[:, 0] = s["x0"]
    return s, m, xs, us


def sweep_reference(m, s, xs, us, b, mode=1):
    """-> (sweep_cases.Sweep, J, {alpha: (xn, un, Jn)}) of instance b, the shape sweep_cases.assert_sweep_matches / _rollout_ take;
    mode = 2: the full second-order tensor of a second_order = 2 build"""
    from oracle import ddp as oddp
    from tests.sweep_cases import Sweep
    P = s["params"][b]
    d = oddp.defects(m, xs[b], us[b], P)
    r = oddp.backward_pass(m, xs[b], us[b], P, d, SWEEP_MU, SWEEP_THETA, mode)
    sw = Sweep(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[9])
    fw = {a: oddp.forward_pass(m, s["x0"][b], xs[b], us[b], P, d, sw.K, sw.kff, a) for a in SWEEP_ALPHAS} if sw.ok else {}
    return sw, oddp.total_cost(m, xs[b], us[b], P), fw


# ---- the table form: every promised field drawn per instance ------------------------------------------------------------------------------
TABLE_B = 6


def draw_all(model, B=TABLE_B, seed=2027, base=None):
    """Per instance, from ONE default_rng(seed), in the order of _lib.INSTANCE_CONST_FIELDS: every scalar x U(0.5, 2) (m x U(0.75,
    1.25), dt and lip_height x U(0.8, 1.25): a robot, not a toy); I = s (I_0 + a symmetric push of up to 10 % of its diagonal), s in
    U(0.8, 1.25); com and feet + U(-0.02, 0.02) per component; inertia_mode, relative_velocity_constraints and lever_sign alternate so
    that both values of each occur, in another pattern each.  -> (overrides for set_instance_consts, [constants dict per instance])"""
    from srbd_horizon_amd import _lib
    base = defaults(model) if base is None else base
    rng = np.random.default_rng(seed)
    narrow = dict(m=(0.75, 1.25), dt=(0.8, 1.25), lip_height=(0.8, 1.25), force_scaling=(0.8, 1.25))
    over = {k: [] for k in _lib.INSTANCE_CONST_FIELDS}
    for b in range(B):
        for k in _lib.INSTANCE_CONST_FIELDS:
            if k == "I":
                I0 = np.asarray(base["I"], dtype=float).reshape(3, 3)
                push = rng.uniform(-0.1, 0.1, (3, 3)) * np.sqrt(np.outer(np.diag(I0), np.diag(I0)))
                v = rng.uniform(0.8, 1.25) * (I0 + 0.5 * (push + push.T))
                assert np.all(np.linalg.eigvalsh(v) > 0.0)
            elif k in ("com", "feet"):
                a = np.asarray(base[k], dtype=float)
                v = a + rng.uniform(-0.02, 0.02, a.shape)
            elif k == "inertia_mode":
                v = b % 2
            elif k == "relative_velocity_constraints":
                v = (b // 2) % 2
            elif k == "lever_sign":
                v = -1.0 if b % 3 == 1 else 1.0
            else:
                v = base[k] * rng.uniform(*narrow.get(k, (0.5, 2.0)))
            over[k].append(v)
    over = {k: np.asarray(v) for k, v in over.items()}
    rows = [dict(base, **{k: (over[k][b] if np.ndim(over[k][b]) else over[k][b].item()) for k in over}) for b in range(B)]
    return over, rows
