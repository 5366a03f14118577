"""What the plan-uncertainty tests share (tests/test_policy_covariance_cpu.py, tests/test_gpu_policy_covariance.py): the rule of
sddp_policy_covariance_device (include/sddp.h), stated once in numpy over the oracle's model Jacobians, the one-step check the GPU
test makes with it, and the record recomputed from the device's own covariances.

THE RULE.  With the plan (xs, us), the parameters P, the exported gains K and the policy record's last word ok of one instance, from
S_0 = S0 at node `start`, for k = start + j, j = 0 .. steps - 1:
    [f_x f_u] = m.f_jac(xs[k], us[k], P[k])       at the STORED knot
    A_k = f_x + f_u K[k]  (ok != 0);   A_k = f_x  (ok == 0: K is not multiplied at all -- whatever it holds);   B_k = f_u
    S_{j+1} = A_k S_j A_k^T + B_k diag(r) B_k^T + diag(q)                          (q, r None: 0)
    U_j = K[k] S_j K[k]^T  (zeros when ok == 0)
Cone margin in standard deviations, where the model's contact forces are inputs: for a stage node k, a contact n in stance there (the
audit's test: tests/plan_audit_cases.py) and row a of oracle.models.friction_cone_rows (ml = coefficient / sqrt(2), the audit's),
    margin = -a . f_k,n,   spread = sqrt(a^T C a),  C the 3 x 3 block of U_j of that force;   spread == 0: skipped;   z = margin / spread.
THE RECORD (16 words; srbd_horizon_amd._lib POLICY_COV_*):
    0  min z, +inf if none counted      1, 2, 3  its node, contact, row (-1: none; first in node-major order on ties)
    4  max_j trace S_j, j = 0 .. steps      5  its node      6  trace S_steps      7  max_i S_steps[i][i]      8  its state index
    9  max over j < steps, r of U_j[r][r]      10, 11  its node, input      12  min over j, i of S_j[i][i]
    13  steps      14  ok      15  0
A NaN operand makes a word NaN and its indices -1.
"""
import numpy as np

from oracle import models as omodels
from srbd_horizon_amd import _lib
from tests import plan_audit_cases as pac

WORDS = _lib.POLICY_COV_WORDS
# the one-step bound: 1e-11 is the knot-level tolerance tests/test_gpu_parity.py test_eval_knots_matches_oracle gives F; x 2 for the two
# factors of A, x 2 for margin.  The rounding of the chains, (2 nx + nu + 2) 2^-53, is far below it.
STEP_TOL = 4e-11
RECORD_RTOL = 1e-11


def linearisation(m, xs, us, P, K, ok, k):
    """-> (A_k, B_k) of the rule"""
    fx, fu = m.f_jac(xs[k], us[k], P[k])
    return (fx + fu @ K[k] if ok else fx), fu


def step(A, B, S, q, r):
    Sn = A @ S @ A.T
    if r is not None:
        Sn = Sn + (B * r) @ B.T
    if q is not None:
        Sn = Sn + np.diag(q)
    return np.tril(Sn) + np.tril(Sn, -1).T          # S'[m][i] is the word of S'[i][m], m <= i: symmetric by construction


def step_bound(A, B, S, q, r):
    bound = np.abs(A) @ np.abs(S) @ np.abs(A).T
    if r is not None:
        bound = bound + (np.abs(B) * np.abs(r)) @ np.abs(B).T
    if q is not None:
        bound = bound + np.diag(np.abs(q))
    return STEP_TOL * bound


def _place(values, keys):
    """the maximum of `values` and the key of its first occurrence; NaN: (nan, None); no candidate: (-inf, None)"""
    if len(values) == 0:
        return -np.inf, None
    v = np.asarray(values, dtype=float)
    if np.isnan(v).any():
        return np.nan, None
    at = int(np.argmax(v))
    return float(v[at]), keys[at]


def cone_candidates(m, us, P, K, ok, cov, start, ml):
    """every counted (node, stance contact, row) of the rule from the covariances cov [steps + 1, nx, nx] -> list of
    (z, node, contact, row, spread) in node-major order; empty where the model has no force inputs or ok == 0"""
    base, w = pac._parts(m)
    out = []
    if w["f"] is None or not ok:
        return out
    rows = omodels.friction_cone_rows(ml * np.sqrt(2.0))
    for j in range(cov.shape[0] - 1):
        k = start + j
        for n in range(w["nc"]):
            if not P[k][w["sw"](n)] > 0.5:
                continue
            Kf = K[k][w["f"](n)]
            C = Kf @ cov[j] @ Kf.T
            f = us[k][w["f"](n)]
            for row, a in enumerate(rows):
                with np.errstate(invalid="ignore"):
                    spread = np.sqrt(a @ C @ a)
                if spread == 0.0:
                    continue
                out.append((-(a @ f) / spread, k, n, row, spread))
    return out


def record_of(m, us, P, K, ok, cov, udiag, start, ml):
    """the record of the rule from covariances cov [steps + 1, nx, nx] and diag U udiag [steps, nu] (the reference's own, or the
    device's) -> (record [16], the cone candidates)"""
    steps = cov.shape[0] - 1
    rec = np.zeros(WORDS)
    cand = cone_candidates(m, us, P, K, ok, cov, start, ml)
    top, at = _place([-c[0] for c in cand], [c[1:4] for c in cand])
    rec[0] = -top
    rec[1:4] = (-1, -1, -1) if at is None else at
    tr = [float(np.sum(np.diag(cov[j]))) for j in range(steps + 1)]
    top, at = _place(tr, list(range(start, start + steps + 1)))
    rec[4], rec[5] = top, -1 if at is None else at
    rec[6] = tr[steps]
    top, at = _place(np.diag(cov[steps]), list(range(m.nx)))
    rec[7], rec[8] = top, -1 if at is None else at
    top, at = _place(udiag.reshape(-1), [(start + j, r) for j in range(steps) for r in range(m.nu)])
    rec[9] = top
    rec[10:12] = (-1, -1) if at is None else at
    d = np.array([np.diag(cov[j]) for j in range(steps + 1)])
    rec[12] = np.nan if np.isnan(d).any() else float(np.min(d))
    rec[13], rec[14], rec[15] = steps, 1.0 if ok else 0.0, 0.0
    return rec, cand


def covariance_reference(m, xs, us, P, K, ok, S0, q, r, start, steps, ml):
    """one instance -> dict(cov [steps + 1, nx, nx], ucov [steps, nu, nu], ucov_diag [steps, nu], record [16], cone: the candidates);
    S0 symmetric (its lower triangle is what counts), K [>= start + steps, nu, nx]"""
    S = np.tril(S0) + np.tril(S0, -1).T
    cov = np.empty((steps + 1, m.nx, m.nx))
    ucov = np.zeros((steps, m.nu, m.nu))
    cov[0] = S
    for j in range(steps):
        k = start + j
        A, B = linearisation(m, xs, us, P, K, ok, k)
        if ok:
            ucov[j] = K[k] @ cov[j] @ K[k].T
        cov[j + 1] = step(A, B, cov[j], q, r)
    udiag = np.array([np.diag(u) for u in ucov]).reshape(steps, m.nu)
    rec, cand = record_of(m, us, P, K, ok, cov, udiag, start, ml)
    return dict(cov=cov, ucov=ucov, ucov_diag=udiag, record=rec, cone=cand)


def assert_one_step(m, xs, us, P, K, ok, q, r, start, got_cov, label=""):
    """The device's covariances got_cov [steps + 1, nx, nx] of one instance against the rule, knot by knot FROM THE DEVICE'S OWN S_j, so
    nothing compounds: |S_{j+1} - (A S_j A^T + B diag(r) B^T + diag(q))| <= STEP_TOL (|A| |S_j| |A|^T + |B| diag(r) |B|^T + diag(q)),
    entrywise; every S_j exactly symmetric.  -> the worst error / bound, for printing."""
    worst = 0.0
    for j in range(got_cov.shape[0] - 1):
        k = start + j
        A, B = linearisation(m, xs, us, P, K, ok, k)
        ref, bound = step(A, B, got_cov[j], q, r), step_bound(A, B, got_cov[j], q, r)
        err = np.abs(got_cov[j + 1] - ref)
        assert np.array_equal(got_cov[j + 1], got_cov[j + 1].T), f"{label} knot {k}: S is not symmetric"
        bad = err > bound
        assert not bad.any(), f"{label} knot {k}: {int(bad.sum())} entries off, worst {float(np.max(err[bad] / np.maximum(bound[bad], 1e-300))):.3e} x the bound"
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    return worst


def assert_record(m, us, P, K, ok, start, ml, got_rec, got_cov, got_udiag, label=""):
    """The device's record against the rule's words recomputed from the device's OWN covariances and diag U (and the fetched K), at
    RECORD_RTOL; word 0 and its place where the reference counted a triple (its own spread non-zero), exactly +inf / -1 where it counted
    none; the index words exactly, or -- under a tie within the tolerance -- a place whose candidate is within it of the best."""
    ref, cand = record_of(m, us, P, K, ok, got_cov, got_udiag, start, ml)
    assert got_rec.shape == (WORDS,), (label, got_rec.shape)
    steps = got_cov.shape[0] - 1
    for w in (4, 6, 7, 9, 12):
        np.testing.assert_allclose(got_rec[w], ref[w], rtol=RECORD_RTOL, atol=0.0, err_msg=f"{label} word {w}")
    for w in (13, 14, 15):
        assert got_rec[w] == ref[w], f"{label} word {w}: {got_rec[w]} against {ref[w]}"
    tr = np.array([np.sum(np.diag(got_cov[j])) for j in range(steps + 1)])
    node = int(got_rec[5])
    assert start <= node <= start + steps and tr[node - start] >= ref[4] * (1 - RECORD_RTOL) - 0.0, f"{label} word 5: {got_rec[5]}"
    idx = int(got_rec[8])
    assert 0 <= idx < m.nx and got_cov[steps][idx, idx] >= ref[7] - RECORD_RTOL * abs(ref[7]), f"{label} word 8: {got_rec[8]}"
    node, r = int(got_rec[10]), int(got_rec[11])
    assert start <= node < start + steps and 0 <= r < m.nu and got_udiag[node - start, r] >= ref[9] - RECORD_RTOL * abs(ref[9]), \
        f"{label} words 10, 11: {got_rec[10:12]}"
    if not cand:
        assert got_rec[0] == np.inf and tuple(got_rec[1:4]) == (-1, -1, -1), f"{label}: no triple counted, the device has {got_rec[:4]}"
        return ref
    np.testing.assert_allclose(got_rec[0], ref[0], rtol=RECORD_RTOL, atol=0.0, err_msg=f"{label} word 0")
    at = [c for c in cand if c[1:4] == tuple(int(v) for v in got_rec[1:4])]
    assert at and at[0][0] <= ref[0] + RECORD_RTOL * abs(ref[0]), f"{label} words 1 - 3: {got_rec[1:4]} holds {at}, the minimum is {ref[0]}"
    return ref


def general_s0(nx, seed, scale=1e-4):
    """a full, non-diagonal symmetric positive definite [nx, nx]"""
    g = np.random.default_rng(seed).standard_normal((nx, nx))
    return scale * (g @ g.T / nx + 0.5 * np.eye(nx))


def transition_matrix(rollout, x0, h=1.0):
    """Phi of an AFFINE map x0 -> rollout(x0) by central differences: column i = (rollout(x0 + h e_i) - rollout(x0 - h e_i)) / (2 h),
    exact to rounding"""
    cols = []
    for i in range(x0.size):
        e = np.zeros(x0.size)
        e[i] = h
        cols.append((rollout(x0 + e) - rollout(x0 - e)) / (2.0 * h))
    return np.array(cols).T


# The rounding of S_steps = Phi S0 Phi^T on the reference alone, on the lip30 problem the GPU test runs (tests/plan_audit_cases.py problem
# ("lip30", 6, 3, "plain"): linear, so the identity is exact): the oracle's plans with the gains of tests/policy_cases.py (max |K| = 345),
# five S0 each, Phi by central differences of the rollout at h = 1 around the plan.  max |S_N - Phi S0 Phi^T| / max |S_N| was at most
# 9.1e-15.  The tolerance is that with a margin of x 10, and it is the one that holds the device's covariance to the device's own
# rollout in tests/test_gpu_policy_covariance.py.
LIP_IDENTITY_MEASURED = 9.1e-15
LIP_IDENTITY_TOL = 10.0 * LIP_IDENTITY_MEASURED


def identity_error(S_N, Phi, S0):
    return float(np.max(np.abs(S_N - Phi @ S0 @ Phi.T)) / np.max(np.abs(S_N)))
