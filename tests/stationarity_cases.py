"""What the stationarity tests share (tests/test_stationarity_cpu.py, tests/test_gpu_stationarity.py): the record and the full outputs of
sddp_stationarity_range_device (include/sddp.h), stated once in numpy over the oracle's models, the comparison of a device result with
it, and the cases.

THE RECURSION for one instance, from a trajectory x [N + 1, nx], u [N, nu] and the parameters P [N + 1, np]:
    lambda_N = l_x,N;   q_k = [l_x,k ; l_u,k] + F_k^T lambda_{k+1},  F_k = [f_x f_u] at (x_k, u_k, p_k),  k = N - 1 .. 0
    lambda_k = q_k[0:nx];   s_k = q_k[nx:nz]
entry z of q_k starting at g[z] and adding F[j][z] lambda_{k+1}[j] for j = 0 .. nx - 1 in this order (the device fuses each step).
THE RECORD (8 doubles, _lib.STATIONARITY_FIELDS):
    0  max over k, i of |s_k[i]|      1, 2  its node and input (the first in node-major order on ties; -1 where word 0 is NaN)
    3  max over k, i of |l_u,k[i]| + sum_j |F_k[j][nx + i]| |lambda_{k+1}[j]|      4  max |lambda_0|      5  max over k >= 1 of |lambda_k|
    6  max over k of ||x_{k+1} - f(x_k, u_k; p_k)||_inf      7  N
Every maximum propagates NaN (numpy's does).
"""
import functools

import numpy as np

from oracle import cport, models as omodels
from srbd_horizon_amd import _lib
from tests import oracle_refs as refs, plan_audit_cases as pac

W = len(_lib.STATIONARITY_FIELDS)
STAT, NODE, INPUT, SCALE, LAM0, LAM_MAX, DEFECT, NODES = range(8)

# the audit's shapes (tests/plan_audit_cases.py): the smallest at which every model and build kind runs; nz below and above 64
OPTS = pac.OPTS
CASES = pac.CASES
PLAIN = tuple(c for c in CASES if c[3] == "plain")
# The seeds of srbd_horizon_amd.workload per case.  srbd13: the audit's 3 .. B + 2.  srbd37 and srbd61 are symmetric robots: on most seeds
# the two largest |s| of the SOLVED plan are equal to the last bit or exactly (two contacts of one foot), which leaves the place of word 0
# to rounding; these seeds are the first of 0 .. 23 on which they differ by more than 1e-9 (srbd37) / 1e-11 (srbd61) of word 3.
SEEDS = {("srbd13", "plain"): (3, 4, 5, 6, 7), ("srbd37", "plain"): (3, 8, 14), ("lip30", "plain"): (3, 4, 5), ("srbd61", "plain"): (9, 11),
         ("srbd13", "x"): (3, 4, 5), ("srbd13", "bar"): (3, 4, 5, 6, 7), ("srbd13", "so2"): (3, 4, 5, 6, 7)}


def problem(model, N, B, kind):
    """-> (batch, P, consts, opts) of a case (tests/plan_audit_cases.py problem, on SEEDS)"""
    return pac.problem(model, N, B, kind, SEEDS[model, kind])


# ---- the two CPU statements of the derivatives ---------------------------------------------------------------------------------------------
def model_terms(model):
    """(k, x, u, p, terminal) -> (g [nz], F [nx, nz] or None) from oracle.models: cost_derivs and f_jac"""
    def terms(k, x, u, p, terminal):
        if terminal:
            lx = model.cost_derivs(x, None, p, k)[1]
            return np.concatenate([lx, np.zeros(model.nu)]), None
        _, lx, lu, *_ = model.cost_derivs(x, u, p, k)
        return np.concatenate([lx, lu]), np.hstack(model.f_jac(x, u, p))
    return terms


def cport_terms(name, cst):
    """the same from the derivative outputs (F, g) of the C port's knot evaluation (oracle/cport.py eval_knot)"""
    nu = cport.DIMS[name][1]

    def terms(k, x, u, p, terminal):
        _, F, _, g, _ = cport.eval_knot(cst, x, np.zeros(nu) if terminal else u, p, k, terminal, name)
        return g, (None if terminal else F)
    return terms


def reference(terms, f, x, u, P):
    """-> (record [8], lambda [N + 1, nx], s [N, nu], cand [N, nu] = |s|).  terms: model_terms / cport_terms; f(x, u, p): the model step."""
    x, u, P = np.asarray(x, dtype=float), np.asarray(u, dtype=float), np.asarray(P, dtype=float)
    N, nu = u.shape
    nx = x.shape[1]
    lam, s, mag = np.zeros((N + 1, nx)), np.zeros((N, nu)), np.zeros((N, nu))
    defect = np.zeros(N)
    with np.errstate(invalid="ignore", over="ignore"):
        lam[N] = terms(N, x[N], None, P[N], True)[0][:nx]
        for k in range(N - 1, -1, -1):
            g, F = terms(k, x[k], u[k], P[k], False)
            q, m = g.copy(), np.abs(g)
            for j in range(nx):
                q = q + F[j] * lam[k + 1, j]
                m = m + np.abs(F[j]) * abs(lam[k + 1, j])
            lam[k], s[k], mag[k] = q[:nx], q[nx:], m[nx:]
            defect[k] = np.max(np.abs(x[k + 1] - f(x[k], u[k], P[k])))
    cand = np.abs(s)
    rec = np.zeros(W)
    rec[STAT] = np.max(cand)
    at = -1 if np.isnan(rec[STAT]) else int(np.argmax(cand.reshape(-1) == rec[STAT]))
    rec[NODE], rec[INPUT] = (-1, -1) if at < 0 else divmod(at, nu)
    rec[SCALE], rec[LAM0], rec[LAM_MAX] = np.max(mag), np.max(np.abs(lam[0])), np.max(np.abs(lam[1:]))
    rec[DEFECT], rec[NODES] = np.max(defect), N
    return rec, lam, s, cand


def model_reference(model, x, u, P):
    return reference(model_terms(model), model.f, x, u, P)


def relative(rec):
    """word 0 / word 3: the relative measure"""
    return rec[..., STAT] / rec[..., SCALE]


# ---- tolerance: what two correct float64 statements of the same recursion differ by --------------------------------------------------------
def disagreement(name, cst, x, u, P):
    """The recursion twice on one instance, from oracle.models and from the C port's (F, g) -> (ds, dlam, dscale, tie):
    ds    largest |difference| of s and of word 0, over word 3        dlam  largest |difference| of lambda and of words 4, 5, over word 5
    dscale  |difference| of word 3, over word 3
    tie   (largest - second largest candidate of word 0) / word 3: a place is decided only where this exceeds the tolerance"""
    m = omodels.make_model(name, cst)
    a, la, sa, cand = reference(model_terms(m), m.f, x, u, P)
    b, lb, sb, _ = reference(cport_terms(name, cst), m.f, x, u, P)
    ds = max(np.max(np.abs(sa - sb)), abs(a[STAT] - b[STAT])) / a[SCALE]
    dlam = max(np.max(np.abs(la - lb)), abs(a[LAM0] - b[LAM0]), abs(a[LAM_MAX] - b[LAM_MAX])) / a[LAM_MAX]
    top = np.sort(cand.reshape(-1))[-2:]
    return float(ds), float(dlam), float(abs(a[SCALE] - b[SCALE]) / a[SCALE]), float((top[1] - top[0]) / a[SCALE])


@functools.lru_cache(maxsize=None)
def oracle_plans(model, N, B, kind):
    """(batch, P, RobotConsts, xs, us, stats) of a case: the plans the C oracle returns at the case's options; read-only"""
    batch, P, consts, opts = problem(model, N, B, kind)
    cst = omodels.RobotConsts(**consts)
    xs, us, st = refs.c_oracle(model, batch, opts, cst=cst, params=P)
    return batch, refs.frozen(P), cst, xs, us, st


def measure():
    """disagreement over CASES, on the warm starts and on the C oracle's plans -> per case (max ds, max dlam, max dscale, min tie,
    max f_disagreement), and the maxima.  The literals below are its output:
        python -c "from tests import stationarity_cases as sc; sc.measure()"
    """
    worst = np.zeros(4)
    ties = []
    for case in CASES:
        model, N, B, kind = case
        batch, P, cst, xs, us, _ = oracle_plans(*case)
        rows = []
        for x, u in ((batch["xs"], batch["us"]), (xs, us)):
            for b in range(B):
                rows.append(disagreement(model, cst, x[b], u[b], P[b]) + (pac.f_disagreement(model, cst, x[b], u[b], P[b]),))
        r = np.array(rows)
        ties += list(r[:, 3])
        print(f"{model} {kind}: s {r[:, 0].max():.3e}  lambda {r[:, 1].max():.3e}  scale {r[:, 2].max():.3e}  smallest tie gap {r[:, 3].min():.3e}  "
              f"f {r[:, 4].max():.3e}")
        worst = np.maximum(worst, r[:, [0, 1, 2, 4]].max(axis=0))
    print(f"maxima: s {worst[0]!r}  lambda {worst[1]!r}  scale {worst[2]!r}  f {worst[3]!r};  smallest tie gap {min(ties)!r}")
    return worst, np.array(ties)


# Measured by measure() (the command in its docstring) over CASES, on the warm starts and on the C oracle's plans, 2 x 26 instances:
#   srbd13 plain: s 1.898e-16  lambda 4.314e-16  scale 1.898e-16  smallest tie gap 9.098e-08  f 4.441e-16
#   srbd37 plain: s 2.035e-16  lambda 3.058e-16  scale 4.070e-16  smallest tie gap 1.728e-09  f 9.714e-17
#   lip30 plain:  s 5.710e-20  lambda 3.732e-20  scale 0.000e+00  smallest tie gap 4.725e-17  f 9.021e-17
#   srbd61 plain: s 5.854e-17  lambda 5.499e-17  scale 0.000e+00  smallest tie gap 6.159e-11  f 8.327e-17
#   srbd13 x:     s 1.564e-16  lambda 4.490e-16  scale 0.000e+00  smallest tie gap 9.111e-08  f 4.441e-16
#   srbd13 bar:   s 1.898e-16  lambda 4.314e-16  scale 1.898e-16  smallest tie gap 9.098e-08  f 4.441e-16
#   srbd13 so2:   s 1.898e-16  lambda 4.314e-16  scale 3.946e-16  smallest tie gap 1.134e-10  f 4.441e-16
S_DISAGREEMENT = 2.0350052627427925e-16          # s and word 0, over word 3
LAMBDA_DISAGREEMENT = 4.489648465263585e-16      # lambda and words 4, 5, over word 5
SCALE_DISAGREEMENT = 4.070010525485585e-16       # word 3, over word 3
F_DISAGREEMENT = 4.440892098500626e-16           # plan_audit_cases.f_disagreement on the same trajectories (the warm starts give the maximum)
# The device compiles with FMA contraction and fuses every step of the fixed-order sum; the two CPU statements differ by exactly such
# effects (the order of the sums inside the derivatives, the C port's own temporaries), so the GPU tests allow 64 x each figure.
MARGIN = 64.0
S_TOL, LAMBDA_TOL, SCALE_TOL = MARGIN * S_DISAGREEMENT, MARGIN * LAMBDA_DISAGREEMENT, MARGIN * SCALE_DISAGREEMENT      # relative
DEFECT_TOL = 10.0 * F_DISAGREEMENT               # absolute, the audit's rule for its word 10 (plan_audit_cases.DEFECT_TOL)
# A PLACE (words 1, 2) is decided where the two largest |s| differ by more than S_TOL x word 3.  Share of the 52 trajectories above where
# they do not: 3 / 52, the three lip30 plans.  lip30 is linear-quadratic and its solve ends ON the stationary point: word 0 / word 3 of those
# plans is 1.2e-15 .. 2.0e-15, below S_TOL itself, so all of s is rounding there and no seed can decide a place.  On every trajectory whose
# word 0 exceeds S_TOL x word 3 the share is 0 (tests/test_stationarity_cpu.py asserts both statements).


def assert_result(got, lam, s, ref, label="", s_tol=S_TOL, lambda_tol=LAMBDA_TOL, scale_tol=SCALE_TOL, defect_tol=DEFECT_TOL):
    """One device result -- record got [8], lam [N + 1, nx] or None, s [N, nu] or None -- against reference()'s (record, lambda, s, cand).
    s and word 0: |difference| <= s_tol x word 3;  lambda and words 4, 5: <= lambda_tol x word 5;  word 3: <= scale_tol x word 3;  word 6:
    <= defect_tol;  word 7 exactly.  NaN must meet NaN.  Words 1, 2: -1 exactly where the reference has -1; else equal to the
    reference's, unless the reference's two largest candidates lie within s_tol x word 3 of each other -- then the candidate at the
    reported place must lie within that of the maximum.
    -> the worst |difference| / tolerance of (s, lambda), for printing."""
    rec, rlam, rs, cand = ref
    got = np.asarray(got)
    assert got.shape == (W,), (label, got.shape)
    worst = [0.0, 0.0]

    def close(a, b, tol, what, slot=None):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        assert a.shape == b.shape, f"{label} {what}: shape {a.shape} against {b.shape}"
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan), f"{label} {what}: NaN in other places than the reference's"
        d = float(np.max(np.abs(a - b)[~nan], initial=0.0))
        assert d <= tol, f"{label} {what}: |difference| {d:.3e} > {tol:.3e}"
        if slot is not None and tol > 0.0:
            worst[slot] = max(worst[slot], d / tol)

    scale, lmax = rec[SCALE], rec[LAM_MAX]
    if np.isnan(scale) or np.isnan(lmax):                   # a NaN trajectory: the NaN pattern of the record is all that can be compared
        assert np.array_equal(np.isnan(got), np.isnan(rec)), f"{label}: NaN words {np.flatnonzero(np.isnan(got))} against {np.flatnonzero(np.isnan(rec))}"
        if np.isnan(rec[STAT]):
            assert got[NODE] == -1 and got[INPUT] == -1, f"{label}: index words {got[NODE]}, {got[INPUT]} of a NaN maximum"
        assert got[NODES] == rec[NODES]
        return tuple(worst)
    close(got[STAT], rec[STAT], s_tol * scale, "word 0", 0)
    close(got[SCALE], rec[SCALE], scale_tol * scale, "word 3")
    close(got[LAM0], rec[LAM0], lambda_tol * lmax, "word 4", 1)
    close(got[LAM_MAX], rec[LAM_MAX], lambda_tol * lmax, "word 5", 1)
    close(got[DEFECT], rec[DEFECT], defect_tol, "word 6")
    assert got[NODES] == rec[NODES], f"{label} word 7: {got[NODES]} against {rec[NODES]}"
    if s is not None:
        close(s, rs, s_tol * scale, "s", 0)
    if lam is not None:
        close(lam, rlam, lambda_tol * lmax, "lambda", 1)
    if rec[NODE] == -1:
        assert got[NODE] == -1 and got[INPUT] == -1, f"{label}: index words {got[NODE]}, {got[INPUT]}, the reference has none"
    elif (got[NODE], got[INPUT]) != (rec[NODE], rec[INPUT]):
        k, i = int(got[NODE]), int(got[INPUT])
        assert k == got[NODE] and i == got[INPUT] and 0 <= k < cand.shape[0] and 0 <= i < cand.shape[1], f"{label}: index words {got[NODE]}, {got[INPUT]}"
        assert cand[k, i] >= rec[STAT] - s_tol * scale, \
            f"{label}: place ({k}, {i}) holds {cand[k, i]!r}, the maximum {rec[STAT]!r} is at ({int(rec[NODE])}, {int(rec[INPUT])})"
    return tuple(worst)


def place_decided(ref, s_tol=S_TOL):
    """whether the two largest candidates of word 0 differ by more than the tolerance (assert_result then asks for the reference's place)"""
    rec, _, _, cand = ref
    top = np.sort(cand.reshape(-1))[-2:]
    return bool(top[1] - top[0] > s_tol * rec[SCALE])


# ---- the NLP fixtures (tests/nlp_fixtures.py): KKT points found without any DDP code --------------------------------------------------------
def fixture_records(fx):
    """-> (record at the fixture's optimum x / u, record at its start xs0 / us0), from oracle.models"""
    m = omodels.make_model(fx["model"], omodels.RobotConsts(**fx["consts"]))
    return model_reference(m, fx["x"], fx["u"], fx["params"])[0], model_reference(m, fx["xs0"], fx["us0"], fx["params"])[0]


def measure_fixtures():
    """word 0 / word 3 and word 6 at every fixture's optimum and start.  FIXTURE_RECORDS below is its output:
        python -c "from tests import stationarity_cases as sc; sc.measure_fixtures()"
    """
    from tests import nlp_fixtures as nf
    for fx in nf.load_all():
        opt, start = fixture_records(fx)
        print(f'    "{fx["name"]}": ({relative(opt):.3e}, {opt[DEFECT]:.3e}, {relative(start):.3e}, {start[DEFECT]:.3e}),')


# name -> (word 0 / word 3 at the optimum, word 6 at the optimum, word 0 / word 3 at the start, word 6 at the start), as measured
FIXTURE_RECORDS = {
    "nlp_lip30_n20_seed5": (1.056e-14, 3.704e-16, 1.000e+00, 5.866e-03),
    "nlp_srbd13_n30_seed0": (3.191e-16, 8.708e-16, 9.987e-01, 5.502e+00),
    "nlp_srbd13_n30_seed1": (1.921e-16, 3.422e-16, 1.000e+00, 1.433e-01),
    "nlp_srbd13_n30_seed12": (2.127e-16, 4.330e-15, 9.970e-01, 7.474e+00),
    "nlp_srbd13_n30_seed5": (1.492e-16, 2.852e-15, 9.975e-01, 5.510e+00),
    "nlp_srbd37_n20_seed0": (8.290e-16, 2.893e-16, 9.991e-01, 1.111e-01),
    "nlp_srbd37_n20_seed3": (2.455e-16, 3.391e-16, 9.977e-01, 1.304e-01),
    "nlp_srbd37_n60_seed2": (3.308e-14, 1.218e-13, 9.981e-01, 2.351e-01),
    "nlp_srbd37x_n20_seed1": (3.401e-16, 1.052e-15, 1.000e+00, 1.433e-01),
    "nlp_srbd61_n20_seed1": (2.776e-16, 4.111e-16, 1.000e+00, 1.433e-01),
}
