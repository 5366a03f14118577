"""What the plan-audit tests share (tests/test_plan_audit_cpu.py, tests/test_gpu_plan_audit.py): the record of
sddp_audit_range_device (include/sddp.h), stated once in numpy over the oracle's models, and the comparison of a device record with it.

THE RECORD of one instance, from a trajectory x [steps + 1, nx], u [steps, nu] whose row j sits at node start + j, the parameters P
[N + 1, np] and the ground's friction coefficient; ml = coefficient / sqrt(2) (oracle.models.friction_cone_rows).  Stage nodes are
start + j, j < steps; state nodes start + j, j <= steps; contact i is in stance at a node iff its switch parameter there is > 0.5.
    0  cone   max over stage nodes and stance contacts of max(|f_x|, |f_y|) - ml f_z; -inf without one     1, 2  its node, contact
    3  pull   max over stage nodes and stance contacts of -f_z; -inf without one                           4  its node
    5  swing load   max over stage nodes and contacts not in stance of max_a |f_a|; 0 without one
    6  quaternion drift   max over state nodes of | ||o|| - 1 |
    7  foot height   max over stage nodes and contacts of |c_z - c_ref|
    8  slip   max over stage nodes and stance contacts of max(|cdot_x|, |cdot_y|)
    9  rigid foot   max over stage nodes and the pairs of _contact_penalty_rows of |cdot_lead,xy - cdot_i,xy|; 0 without the rows
   10  defect   max over stage nodes of ||x_{k+1} - f(x_k, u_k; p_k)||_inf                                11  its node
   12  stage nodes      13  stance (node, contact) pairs      14, 15  0
srbd13 has its contacts as parameters (7 - 9 are 0); lip30 has neither forces nor a quaternion (0, 3: -inf; 1, 2, 4: -1; 5, 6, 13: 0).
Every maximum propagates NaN (numpy's does), and the index words of a NaN maximum are -1.
"""
import numpy as np

from srbd_horizon_amd import _lib

EPS = np.finfo(np.float64).eps
# words whose operands are fetched numbers combined by at most three products and a sum (the GPU test bounds them by 8 eps x the
# operand sum); the indexed ones among them, with their index words
DIRECT = (_lib.AUDIT_CONE, _lib.AUDIT_PULL, _lib.AUDIT_SWING_LOAD, _lib.AUDIT_QUAT_DRIFT, _lib.AUDIT_FOOT_HEIGHT, _lib.AUDIT_SLIP,
          _lib.AUDIT_RIGID_FOOT)


# ---- the solved cases of tests/test_gpu_plan_audit.py (the shapes of tests/test_gpu_policy_rollout.py) -------------------------------
OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
# (model, N, B, kind): "plain"; "x": the _x build (tests/variant_cases.py rows); "bar": friction barrier on; "so2": second_order = 2
CASES = (("srbd13", 6, 5, "plain"), ("srbd37", 6, 3, "plain"), ("lip30", 6, 3, "plain"), ("srbd61", 4, 2, "plain"), ("srbd13", 6, 3, "x"),
         ("srbd13", 6, 5, "bar"), ("srbd13", 6, 5, "so2"))


def problem(model, N, B, kind, seeds=None):
    """-> (batch, P, consts, opts) of a case of the plan inspectors' tests (audit, stationarity, cost breakdown) on `seeds` of
    srbd_horizon_amd.workload, None: 3 .. B + 2.  Beyond the kinds of CASES, "lin" and "box": the _x build on the rows, the bound
    barrier on the band of tests/cost_terms_cases.py."""
    from srbd_horizon_amd import workload
    from tests import cost_terms_cases as cc
    from tests.variant_cases import extra_rows
    seeds = np.arange(B) + 3 if seeds is None else np.asarray(seeds)
    assert len(seeds) == B
    batch = workload.make_batch(model, N, seeds)
    P = batch["params"]
    consts = dict(batch["consts"], **(dict(extra_rows=extra_rows(model)) if kind == "x" else cc.consts_of(model, "x" if kind == "lin" else kind)))
    if kind in ("x", "lin"):      # the rows' per-knot references: eight more parameter columns, two of them in use
        P = np.concatenate([P, np.zeros((B, N + 1, 8))], axis=2)
        P[:, :, P.shape[2] - 8] = 0.02 * np.sin(np.arange(N + 1) / 5.0)[None]
        P[:, :, P.shape[2] - (5 if kind == "x" else 6)] = 0.1 * np.cos(np.arange(N + 1) / 3.0)[None]
    return batch, P, consts, dict(OPTS, **(dict(second_order=2) if kind == "so2" else {}))


def f_disagreement(name, cst, x, u, P):
    """max over the stage nodes of an instance of |oracle.models f - the C port's f| (oracle/cport.py eval_knot) on the same
    (x_k, u_k, p_k): what two correct float64 statements of the model step differ by."""
    from oracle import cport, models as omodels
    m = omodels.make_model(name, cst)
    return max(float(np.max(np.abs(m.f(x[k], u[k], P[k]) - cport.eval_knot(cst, x[k], u[k], P[k], k, False, name)[0]))) for k in range(u.shape[0]))


# f_disagreement measured on the CPU over CASES: on the plans the C oracle returns for them (oracle.cport.solve_batch at OPTS) it is at
# most 9.03e-17, and on 20 copies of those plans pushed by 1e-2 N(0, 1) per state entry -- the states a policy rollout from a pushed
# state visits -- at most 2.23e-16 (one ulp of 1, on srbd13 "so2").  The larger figure is the one the defect's tolerance is built on.
F_DISAGREEMENT = 2.220446049250313e-16
DEFECT_TOL = 10.0 * F_DISAGREEMENT      # the margin of 10 covers another contraction order on the device


def _parts(model):
    """the model behind a user-row wrapper, and where it keeps what the audit reads"""
    m = getattr(model, "base", model)
    if m.name == "srbd13":
        return m, dict(nc=2, sw=lambda i: m.P_SW[i], f=lambda i: slice(3 * i, 3 * i + 3), quat=m.O_, states=False)
    if m.name == "lip30":
        return m, dict(nc=4, sw=m.p_sw, f=None, quat=None, states=True)
    return m, dict(nc=m.nc, sw=m.p_sw, f=lambda i: slice(6 * i + 3, 6 * i + 6), quat=m.O_, states=True)


def rigid_pairs(m):
    """(lead, other) contact pairs of the relative-velocity rows, as oracle.models._contact_penalty_rows pairs them"""
    cm = m.contact_model if m.cst.relative_velocity_constraints else 1
    return [(0, i) for i in range(1, cm)] + [(cm, i) for i in range(cm + 1, 2 * cm)] if cm > 1 else []


def audit_reference(model, x, u, P, start, friction):
    """-> (record [16], opsum [16], values).
    opsum[w]: for the maxima, the largest absolute operand sum among the candidates of word w (two maxima over candidates that differ
    by at most t each differ by at most t, so a rounding bound on every candidate bounds the maximum); 0 elsewhere.
    values: dict(cone [steps, nc], pull [steps, nc], defect [steps]) -- every candidate of the indexed words (nan-free entries only
    where the contact is in stance; -inf elsewhere), for checking a reported place under ties."""
    m, w = _parts(model)
    x, u, P = np.asarray(x, dtype=float), np.asarray(u, dtype=float), np.asarray(P, dtype=float)
    steps, nc = u.shape[0], w["nc"]
    assert x.shape[0] == steps + 1 and steps >= 1 and start >= 0 and start + steps <= P.shape[0] - 1
    ml = friction / np.sqrt(2.0)
    rec, ops = np.zeros(_lib.AUDIT_WORDS), np.zeros(_lib.AUDIT_WORDS)
    cone = np.full((steps, nc), -np.inf); pull = np.full((steps, nc), -np.inf); defect = np.zeros(steps)
    cone_ops = np.zeros((steps, nc)); pull_ops = np.zeros((steps, nc))
    swing, drift, height, slip, rigid = [0.0], [0.0], [0.0], [0.0], [0.0]
    swing_o, drift_o, height_o, slip_o, rigid_o = [0.0], [0.0], [0.0], [0.0], [0.0]
    pairs = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(steps + 1):
            if w["quat"] is not None:
                n = np.sqrt(np.sum(x[j, w["quat"]] ** 2))
                drift.append(abs(n - 1.0)); drift_o.append(abs(n) + 1.0)
            if j == steps:
                break
            p = P[start + j]
            for i in range(nc):
                stance = p[w["sw"](i)] > 0.5
                if w["f"] is not None:
                    f = u[j, w["f"](i)]
                    side = np.max(np.abs(f[0:2]))
                    if stance:
                        cone[j, i] = side - ml * f[2]; cone_ops[j, i] = side + abs(ml * f[2])
                        pull[j, i] = -f[2]; pull_ops[j, i] = abs(f[2])
                        pairs += 1
                    else:
                        swing.append(np.max(np.abs(f))); swing_o.append(swing[-1])
                if w["states"]:
                    cz, cref = x[j, m.C_IDX[i] + 2], p[m.p_cref(i)]
                    height.append(abs(cz - cref)); height_o.append(abs(cz) + abs(cref))
                    if stance:
                        slip.append(np.max(np.abs(x[j, m.CD_IDX[i]:m.CD_IDX[i] + 2]))); slip_o.append(slip[-1])
            if w["states"]:
                for a, b in rigid_pairs(m):
                    va, vb = x[j, m.CD_IDX[a]:m.CD_IDX[a] + 2], x[j, m.CD_IDX[b]:m.CD_IDX[b] + 2]
                    rigid.append(np.max(np.abs(va - vb))); rigid_o.append(np.max(np.abs(va) + np.abs(vb)))
            defect[j] = np.max(np.abs(x[j + 1] - model.f(x[j], u[j], p)))

    def place(v):
        """(maximum, flat index of its first occurrence or -1): nan -> -1, no candidate above -inf at all -> -1"""
        top = np.max(v)
        if np.isnan(top) or (np.isneginf(top) and w["f"] is None):
            return top, -1
        return top, int(np.argmax(v.reshape(-1) == top))

    A = _lib
    top, at = place(cone)
    if pairs == 0:
        at = -1
    rec[A.AUDIT_CONE], rec[A.AUDIT_CONE_NODE], rec[A.AUDIT_CONE_CONTACT] = top, (-1 if at < 0 else start + at // nc), (-1 if at < 0 else at % nc)
    top, at = place(pull)
    if pairs == 0:
        at = -1
    rec[A.AUDIT_PULL], rec[A.AUDIT_PULL_NODE] = top, (-1 if at < 0 else start + at // nc)
    top, at = place(defect)
    rec[A.AUDIT_DEFECT], rec[A.AUDIT_DEFECT_NODE] = top, (-1 if at < 0 else start + at)
    for word, v, o in ((A.AUDIT_SWING_LOAD, swing, swing_o), (A.AUDIT_QUAT_DRIFT, drift, drift_o), (A.AUDIT_FOOT_HEIGHT, height, height_o),
                       (A.AUDIT_SLIP, slip, slip_o), (A.AUDIT_RIGID_FOOT, rigid, rigid_o)):
        rec[word], ops[word] = np.max(v), np.nanmax(o)
    ops[A.AUDIT_CONE], ops[A.AUDIT_PULL] = np.nanmax(cone_ops), np.nanmax(pull_ops)
    rec[A.AUDIT_NODES], rec[A.AUDIT_STANCE_PAIRS] = steps, pairs
    return rec, ops, dict(cone=cone, pull=pull, defect=defect)


def assert_record(got, ref, ops, values, start, defect_tol, label=""):
    """One device record against audit_reference's (record, opsum, values).
    Words 0, 3, 5 - 9: |got - ref| <= 8 eps x opsum (NaN and infinities must agree exactly).  Word 10: |got - ref| <= defect_tol.
    Index words: -1 exactly where the reference has -1 (a NaN or empty maximum); otherwise the reference's candidate AT THE REPORTED
    PLACE is within the word's tolerance of the reference's maximum (which holds under ties).  Words 12 - 15 exactly.
    -> the worst |got - ref| / tolerance over the direct words and over word 10, for printing."""
    A = _lib
    got = np.asarray(got)
    assert got.shape == (A.AUDIT_WORDS,), (label, got.shape)
    worst = [0.0, 0.0]

    def close(word, tol, slot):
        g, r = got[word], ref[word]
        if np.isnan(r) or np.isinf(r):
            assert (np.isnan(g) and np.isnan(r)) or g == r, f"{label} word {word}: {g} against {r}"
            return
        assert abs(g - r) <= tol, f"{label} word {word}: {g!r} against {r!r}, |difference| {abs(g - r):.3e} > {tol:.3e}"
        if tol > 0.0:
            worst[slot] = max(worst[slot], abs(g - r) / tol)

    for word in DIRECT:
        close(word, 8 * EPS * ops[word], 0)
    close(A.AUDIT_DEFECT, defect_tol, 1)
    nc = values["cone"].shape[1]
    for word, node_w, contact_w, cand, tol in ((A.AUDIT_CONE, A.AUDIT_CONE_NODE, A.AUDIT_CONE_CONTACT, values["cone"], 8 * EPS * ops[A.AUDIT_CONE]),
                                               (A.AUDIT_PULL, A.AUDIT_PULL_NODE, None, values["pull"], 8 * EPS * ops[A.AUDIT_PULL]),
                                               (A.AUDIT_DEFECT, A.AUDIT_DEFECT_NODE, None, values["defect"], defect_tol)):
        idx = [got[node_w]] + ([got[contact_w]] if contact_w is not None else [])
        if ref[node_w] == -1:
            assert all(v == -1 for v in idx), f"{label} index words of word {word}: {idx}, the reference has none"
            continue
        node = int(got[node_w])
        assert node == got[node_w] and start <= node < start + cand.shape[0], f"{label} node of word {word}: {got[node_w]}"
        if contact_w is not None:
            c = int(got[contact_w])
            assert c == got[contact_w] and 0 <= c < nc, f"{label} contact of word {word}: {got[contact_w]}"
            there = cand[node - start, c]
        else:
            there = np.max(cand[node - start])        # (pull: the node alone is reported; defect: one candidate per node)
        assert there >= ref[word] - tol, f"{label} word {word}: the place reported holds {there!r}, the maximum is {ref[word]!r}"
    for word in (A.AUDIT_NODES, A.AUDIT_STANCE_PAIRS, 14, 15):
        assert got[word] == ref[word], f"{label} word {word}: {got[word]} against {ref[word]}"
    return tuple(worst)
