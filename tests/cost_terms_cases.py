"""What the cost-breakdown tests share (tests/test_cost_terms_cpu.py, tests/test_gpu_cost_terms.py): the record of
sddp_cost_terms_range_device (include/sddp.h) stated twice in numpy over the oracle's models, the comparison of a device result with
it, and the cases.  Imports `oracle` only.

THE RECORD of one instance, from a trajectory x [N + 1, nx], u [N, nu] and the parameters P [N + 1, np]: 16 doubles,
    0  total      1 + f  family f = 0 .. 12 (NAMES)      14  the largest of the families 0 .. 11 (first on ties, -1 with a NaN)      15  N
each of the words 0 .. 13 the sum over the nodes k = 0 .. N of the node's value, added in node order; `nodes` [N + 1, 14] holds the addends.
Statement A: the node's value of family f is oracle.models' cost(x_k, u_k, p_k, k) of a model whose RobotConsts keep the gains of
  that family and have 0 in every other one (KEEPS; the fixed 1e6 of the constraints is the module's CONSTRAINT_WEIGHT, the user
  rows' weights are those of extra_rows), with the one weight that is a parameter, orientation_tracking_gain, 0 as well; family 12
  keeps no gain and the parameters as they are; the total keeps everything.
Statement B: the rows of the stacked residual(x_k, u_k, p_k, k) of the unmasked model, grouped by family (row_families), squared and
  summed.
"""
import contextlib
import dataclasses
import functools

import numpy as np

from oracle import models as omodels

NAMES = ("r_tracking", "rdot_tracking", "w_tracking", "rel_pos", "min_f", "force_switch", "min_qddot", "zmp_tracking", "constraints",
         "friction_barrier", "bound_barrier", "user_rows", "unweighted")
WORDS, FAMILIES, COLS = 16, 13, 14
TOTAL, LARGEST, NODES = 0, 14, 15
# the RobotConsts fields a family keeps; "CONSTRAINT_WEIGHT" is the module constant, "extra_rows" the weights of the user rows
KEEPS = {0: ("r_tracking_gain",), 1: ("rdot_tracking_gain",), 2: ("w_tracking_gain",), 3: ("rel_pos_gain",), 4: ("min_f_gain",),
         5: ("force_switch_weight",), 6: ("min_qddot_gain",), 7: ("zmp_tracking_gain",), 8: ("CONSTRAINT_WEIGHT",),
         9: ("friction_barrier_weight",), 10: ("bound_barrier_weight",), 11: ("extra_rows",), 12: ()}
GAINS = tuple(KEEPS[f][0] for f in range(8))                 # the eight gains of the parameter server, by family
P_OTG = 6                                                    # orientation_tracking_gain: column 6 of a parameter row of every srbd model
EPS = np.finfo(np.float64).eps


def base_of(model):
    return getattr(model, "base", model)


def masked_consts(cst, f):
    """RobotConsts that keep family f's gains (f None: everything) -> (RobotConsts, CONSTRAINT_WEIGHT to evaluate them under)"""
    if f is None:
        return cst, omodels.CONSTRAINT_WEIGHT
    keep = KEEPS[f]
    over = {g: 0.0 for fam in range(11) for g in KEEPS[fam] if g != "CONSTRAINT_WEIGHT" and g not in keep}
    if cst.extra_rows and "extra_rows" not in keep:
        over["extra_rows"] = tuple(dict(r, w=0.0) for r in cst.extra_rows)
    return dataclasses.replace(cst, **over), (omodels.CONSTRAINT_WEIGHT if "CONSTRAINT_WEIGHT" in keep else 0.0)


@contextlib.contextmanager
def constraint_weight(w):
    old = omodels.CONSTRAINT_WEIGHT
    omodels.CONSTRAINT_WEIGHT = w
    try:
        yield
    finally:
        omodels.CONSTRAINT_WEIGHT = old


def _sum_in_order(nodes):
    acc = np.zeros(nodes.shape[1])
    for row in nodes:
        acc = acc + row
    return acc


def record_of(nodes):
    """the record [16] of the addends nodes [N + 1, 14]"""
    rec = np.zeros(WORDS)
    with np.errstate(invalid="ignore"):
        rec[:COLS] = _sum_in_order(nodes)
    fam = rec[1:1 + FAMILIES - 1]
    rec[LARGEST] = -1.0 if np.isnan(fam).any() else float(np.argmax(fam))
    rec[NODES] = nodes.shape[0] - 1
    return rec


def statement_a(name, cst, x, u, P):
    """-> (record [16], nodes [N + 1, 14]) by masking the gains"""
    x, u, P = (np.asarray(a, dtype=float) for a in (x, u, P))
    N = u.shape[0]
    nodes = np.zeros((N + 1, COLS))
    has_otg = name != "lip30"
    P0 = P.copy()
    if has_otg:
        P0[:, P_OTG] = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for col in range(COLS):
            f = None if col == 0 else col - 1
            c, cw = masked_consts(cst, f)
            m = omodels.make_model(name, c)
            Pf = P if f in (None, 12) else P0
            with constraint_weight(cw):
                for k in range(N + 1):
                    nodes[k, col] = m.cost(x[k], u[k] if k < N else None, Pf[k], k)
    return record_of(nodes), nodes


def row_families(model, terminal, k, p):
    """the family of every row of model.residual(x, u, p, k), in the order oracle.models stacks them"""
    m, c = base_of(model), model.cst
    fam = []
    state, stage = terminal or k >= 1, not terminal
    per_force = [4] * 3 + [5] * 3 + ([9] * 5 if c.friction_barrier_weight > 0.0 else [])
    nz = m.nx + m.nu
    nbound = 0
    if c.bound_barrier_weight > 0.0:
        lb = np.full(nz, -np.inf) if c.lower is None else np.asarray(c.lower, dtype=float)[:nz]
        ub = np.full(nz, np.inf) if c.upper is None else np.asarray(c.upper, dtype=float)[:nz]
        nbound = int(np.isfinite(lb).sum() + np.isfinite(ub).sum())

    def penalties(nc, cm):
        cm = cm if c.relative_velocity_constraints else 1
        return [8] * (4 * (cm - 1) if cm > 1 else 0) + [8] * (3 * nc)

    if m.name == "lip30":
        if state:
            fam += [0] * 3 + [1] * 3
        if stage:
            fam += [7] * 3
        if state:
            fam += [3] * 4
        if stage:
            fam += [6] * 15 + penalties(4, m.contact_model)
    else:
        if state:
            fam += [0] + [12] * 4 + [1] * 3 + [2] * 3
            if m.name != "srbd13":
                fam += [3] * 4
        if stage:
            if m.name == "srbd13":
                fam += [6] * 6 + per_force * 2
            else:
                fam += [6] * (6 + 3 * m.nc) + per_force * m.nc + penalties(m.nc, m.contact_model)
            fam += [10] * nbound
    if model is not m:
        for row in model.rows:
            if (k >= 1) if row["kind"] == "state" else (not terminal):
                fam.append(11)
    return np.asarray(fam, dtype=int)


def statement_b(name, cst, x, u, P):
    """-> (record [16], nodes [N + 1, 14]) by grouping the rows of the residual"""
    x, u, P = (np.asarray(a, dtype=float) for a in (x, u, P))
    N = u.shape[0]
    m = omodels.make_model(name, cst)
    nodes = np.zeros((N + 1, COLS))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(N + 1):
            terminal = k == N
            r = m.residual(x[k], None if terminal else u[k], P[k], k)
            fam = row_families(m, terminal, k, P[k])
            assert fam.shape == r.shape, (name, k, fam.shape, r.shape)
            nodes[k, 0] = float(r @ r)
            for f in range(FAMILIES):
                nodes[k, 1 + f] = float(r[fam == f] @ r[fam == f])
    return record_of(nodes), nodes


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# (name, kind): "plain"; "x": three linear user rows; "bar": friction barrier on; "box": bound barrier on
BARRIER = dict(friction_barrier_weight=1e-3, friction_barrier_sharpness=5.0)
KINDS = (("srbd13", "plain"), ("srbd37", "plain"), ("lip30", "plain"), ("srbd61", "plain"), ("srbd13", "x"), ("srbd37", "x"), ("srbd13", "bar"),
         ("srbd13", "box"))
DIMS = {"srbd13": (13, 6, 19), "srbd37": (37, 24, 19), "lip30": (30, 15, 11), "srbd61": (61, 48, 27)}


def linear_rows(name):
    """three user rows: two state rows, one stage row that reads an input"""
    nx, nu, _ = DIMS[name]
    a0, a1, a2 = np.zeros(nx + nu), np.zeros(nx + nu), np.zeros(nx + nu)
    a0[0], a0[1] = 1.0, -0.5
    a1[2] = 1.0
    a2[nx + nu - 1], a2[0] = 1.0, 0.25
    return (dict(a=a0, w=30.0, kind="state", const=0.01), dict(a=a1, w=200.0, kind="state", const=0.85), dict(a=a2, w=0.5, kind="stage", const=0.0))


def box_bounds(name):
    nx, nu, _ = DIMS[name]
    lo, up = np.full(nx + nu, -np.inf), np.full(nx + nu, np.inf)
    lo[2], up[2] = 0.80, 0.95
    for j in (nx + 2, nx + 5):
        lo[j], up[j] = 0.0, 0.25
    return dict(bound_barrier_weight=1.0, bound_barrier_sharpness=6.0, lower=lo, upper=up)


def consts_of(name, kind):
    """the dict of constants of a case (what DdpEngine and RobotConsts both take)"""
    c = {}
    if kind == "x":
        c["extra_rows"] = linear_rows(name)
    if kind == "bar":
        c.update(BARRIER)
    if kind == "box":
        c.update(box_bounds(name))
    return c


def random_case(name, kind, N, seed):
    """-> (RobotConsts, x [N + 1, nx], u [N, nu], P [N + 1, np]): a random trajectory around initial_state / static_input under a mixed
    stance pattern and a commanded velocity, so that every family the build has is non-zero somewhere"""
    rng = np.random.default_rng(1000 * seed + N)
    cst = omodels.RobotConsts(**consts_of(name, kind))
    m = omodels.make_model(name, cst)
    b = base_of(m)
    P = np.array(m.default_params(N), dtype=float)
    P[:, 0:3] += 0.2 * rng.standard_normal(3)                                   # rdot_ref
    if name != "lip30":
        P[:, 3:6] += 0.1 * rng.standard_normal(3)                               # w_ref
        sw_cols = list(b.P_SW) if name == "srbd13" else [b.p_sw(i) for i in range(b.nc)]
    else:
        sw_cols = [b.p_sw(i) for i in range(4)]
    for j, col in enumerate(sw_cols):                                           # mixed stance: every contact swings at some node
        P[:, col] = (rng.random(N + 1) < 0.7).astype(float)
        P[(j + 1) % (N + 1), col] = 0.0
    if m is not b:
        P[:, b.np_:b.np_ + 3] = 0.05 * rng.standard_normal((N + 1, 3))
    x = m.initial_state()[None] + 0.05 * rng.standard_normal((N + 1, m.nx))
    u = m.static_input()[None] + 0.05 * rng.standard_normal((N, m.nu))
    return cst, x, u, P


def relative_disagreement(a, b):
    """per column 0 .. 13: the largest |difference| of the records and of the addends, over the record's own size (0 where both are 0)"""
    (ra, na), (rb, nb) = a, b
    out = np.zeros(COLS)
    for col in range(COLS):
        scale = max(abs(ra[col]), abs(rb[col]))
        d = max(abs(ra[col] - rb[col]), float(np.max(np.abs(na[:, col] - nb[:, col]))))
        out[col] = 0.0 if d == 0.0 else d / scale
    return out


@functools.lru_cache(maxsize=None)
def measure():
    """A against B over KINDS x N in (3, 5) x seeds 0, 1 -> {column name: the largest relative disagreement}; written by
    tests/test_cost_terms_cpu.py into profiles/cost_terms/cpu_disagreement.json"""
    worst = np.zeros(COLS)
    for name, kind in KINDS:
        for N in (3, 5):
            for seed in (0, 1):
                cst, x, u, P = random_case(name, kind, N, seed)
                worst = np.maximum(worst, relative_disagreement(statement_a(name, cst, x, u, P), statement_b(name, cst, x, u, P)))
    return dict(zip(("total",) + NAMES, (float(v) for v in worst)))


# ---- tolerance of the GPU tests ----------------------------------------------------------------------------------------------------------------
MARGIN = 64.0        # the project's margin for two correct float64 statements of one sum (tests/stationarity_cases.py)


def tolerances(disagreement):
    """per column: MARGIN x the committed CPU disagreement of that column (profiles/cost_terms/cpu_disagreement.json), relative to the
    record's word.  A family the two CPU statements agree on to the bit (0.0) gets one rounding of each of its sum's at most
    N + 1 addends' few products, MARGIN x eps: the statements can agree exactly only where the sum is that short."""
    cols = ("total",) + NAMES
    return np.array([MARGIN * max(disagreement[c], EPS) for c in cols])


def assert_against(got_rec, got_nodes, ref, tol, label=""):
    """a device record [16] and its addends [N + 1, 14] (or None) against a statement's (record, nodes): column c within tol[c] x the
    reference's word c, addends within the same absolute figure; NaN meets NaN; words 14 and 15 exactly unless the two largest families lie
    within their tolerances of each other.  -> the worst |difference| / tolerance, for printing"""
    rec, nodes = ref
    worst = 0.0
    for col in range(COLS):
        bound = tol[col] * abs(rec[col])
        if np.isnan(rec[col]):
            assert np.isnan(got_rec[col]), f"{label} word {col}: {got_rec[col]} where the reference has NaN"
            continue
        d = abs(got_rec[col] - rec[col])
        if got_nodes is not None:
            assert np.array_equal(np.isnan(got_nodes[:, col]), np.isnan(nodes[:, col])), f"{label} column {col}: NaN addends"
            d = max(d, float(np.max(np.abs(got_nodes[:, col] - nodes[:, col]))))
        assert d <= bound, f"{label} word {col} ({(('total',) + NAMES)[col]}): |difference| {d:.3e} > {bound:.3e} (reference {rec[col]:.6e})"
        if bound > 0.0:
            worst = max(worst, d / bound)
    assert got_rec[NODES] == rec[NODES], f"{label} word 15"
    if got_rec[LARGEST] != rec[LARGEST]:
        assert rec[LARGEST] >= 0 and 0 <= got_rec[LARGEST] < FAMILIES - 1 and got_rec[LARGEST] == int(got_rec[LARGEST]), f"{label} word 14: {got_rec[LARGEST]}"
        g, r = 1 + int(got_rec[LARGEST]), 1 + int(rec[LARGEST])
        assert rec[g] >= rec[r] - tol[r] * abs(rec[r]) - tol[g] * abs(rec[g]), f"{label} word 14: family {g - 1} is not the largest ({rec[g]!r} < {rec[r]!r})"
    return worst
