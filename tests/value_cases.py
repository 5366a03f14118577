"""What the cost-to-go tests share (tests/test_value_cpu.py, tests/test_gpu_value.py): the reference of the value records, stated
once in numpy, the comparison, the fixed arithmetic of sddp_value_at_device, and the two experiments.

THE RECORD.  The value export stores, for the nodes k < nodes of an instance, what the policy's sweep (tests/policy_cases.py, THE
RULE: same defects, mu, theta, retry ladder) holds after knot k:
    c_k         the cost of the stored trajectory from node k on: c_N = L_N, c_k = L_k + c_{k+1}, added in this order
    expected_k  -(dV1 + dV2) summed over the knots j >= k; expected_N = 0
    vx_k, Vxx_k Vx / Vxx of oracle/ddp.py backward_pass after knot k (node N: l_x,N and l_xx,N)
and zeros everywhere where the policy record says ok = 0.  value_recursion below is backward_pass with those kept per node: the
same statements in the same order, which tests/test_value_cpu.py pins by comparing its node-0 results with backward_pass's.
"""
from fractions import Fraction

import numpy as np

from oracle import ddp as oddp
from tests import policy_cases as pc


def node_words(nx):
    return nx * nx + nx + 2


def value_recursion(m, xs, us, P, d, mu, theta=0.0, mode=1, L=None):
    """-> ok, dict(c [N+1], expected [N+1], vx [N+1, nx], Vxx [N+1, nx, nx], K [N, nu, nx], kff [N, nu], dV1, dV2).
    L [N + 1]: the per-node costs to sum (default: the model's own, the first result of cost_derivs)."""
    N, nx, nu = us.shape[0], m.nx, m.nu
    out = dict(c=np.zeros(N + 1), expected=np.zeros(N + 1), vx=np.zeros((N + 1, nx)), Vxx=np.zeros((N + 1, nx, nx)),
               K=np.zeros((N, nu, nx)), kff=np.zeros((N, nu)), dV1=0.0, dV2=0.0)
    LN, Vx, _, Vxx, _, _ = m.cost_derivs(xs[N], None, P[N], N)
    out["c"][N] = LN if L is None else L[N]
    out["vx"][N], out["Vxx"][N] = Vx, Vxx
    dV1 = dV2 = 0.0
    for k in range(N - 1, -1, -1):
        fx, fu = m.f_jac(xs[k], us[k], P[k])
        Lk, lx, lu, lxx, lux, luu = m.cost_derivs(xs[k], us[k], P[k], k)
        vp = Vx + Vxx @ d[k]
        Qx = lx + fx.T @ vp
        Qu = lu + fu.T @ vp
        Qxx = lxx + fx.T @ Vxx @ fx
        Qux = lux + fu.T @ Vxx @ fx
        Quu = luu + fu.T @ Vxx @ fu + mu * np.eye(nu)
        if theta and mode == 2:
            S = theta * m.second_order_full(xs[k], us[k], P[k], k, vp)
            Qxx, Qux, Quu = Qxx + S[:nx, :nx], Qux + S[nx:, :nx], Quu + S[nx:, nx:]
        elif theta:
            Qux = Qux + theta * m.second_order_ux(xs[k], us[k], P[k], vp)
        try:
            C = np.linalg.cholesky(Quu)
        except np.linalg.LinAlgError:
            return False, out
        if not np.all(np.diag(C) ** 2 < oddp.PIVOT_MAX):
            return False, out
        sol = -np.linalg.solve(C.T, np.linalg.solve(C, np.column_stack([Qu, Qux])))
        out["kff"][k], out["K"][k] = sol[:, 0], sol[:, 1:]
        kff, K = out["kff"][k], out["K"][k]           # (contiguous rows, as backward_pass multiplies them)
        dV1 += kff @ Qu
        dV2 += 0.5 * kff @ Quu @ kff
        Vx = Qx + Qux.T @ kff
        Vxx = Qxx + Qux.T @ K
        Vxx = 0.5 * (Vxx + Vxx.T)
        out["c"][k] = (Lk if L is None else L[k]) + out["c"][k + 1]
        out["expected"][k] = -(dV1 + dV2)
        out["vx"][k], out["Vxx"][k] = Vx, Vxx
    out["dV1"], out["dV2"] = dV1, dV2
    return True, out


def oracle_values(m, xs, us, P, stats, opt: oddp.DdpOptions, nodes: int, L=None):
    """-> dict(c [nodes], expected [nodes], vx [nodes, nx], Vxx [nodes, nx, nx], ok) by the rule of policy_cases.oracle_policy;
    stats: the solve's record (alpha, gap, mu, status).  L: see value_recursion."""
    N = us.shape[0]
    zeros = dict(c=np.zeros(nodes), expected=np.zeros(nodes), vx=np.zeros((nodes, m.nx)), Vxx=np.zeros((nodes, m.nx, m.nx)), ok=0.0)
    if int(stats["status"]) == 3:
        return zeros
    d = oddp.defects(m, xs, us, P) if float(stats["gap"]) > opt.gap_tol else np.zeros((N, m.nx))
    mu = float(stats["mu"])
    theta = 1.0 if (opt.second_order and float(stats["alpha"]) == opt.alpha_0) else 0.0
    while True:
        ok, v = value_recursion(m, xs, us, P, d, mu, theta, int(opt.second_order) or 1, L)
        if ok:
            return dict(c=v["c"][:nodes].copy(), expected=v["expected"][:nodes].copy(), vx=v["vx"][:nodes].copy(),
                        Vxx=v["Vxx"][:nodes].copy(), ok=1.0)
        if theta:
            theta = 0.0
            continue
        mu = max(mu, 0.0) * 10.0 + opt.mu_min
        if mu > opt.mu_max:
            return zeros


def split_records(rec, nx):
    """raw value records [..., nodes, nx nx + nx + 2] -> dict(c, expected, vx, Vxx)"""
    return dict(c=rec[..., 0], expected=rec[..., 1], vx=rec[..., 2:2 + nx], Vxx=rec[..., 2 + nx:].reshape(*rec.shape[:-1], nx, nx))


def assert_values_match(got, ref, label=""):
    """one instance (dict of split_records) against oracle_values' result, at the tolerance the project uses for one backward sweep
    (policy_cases.assert_policy_matches: rtol 1e-7, atol 1e-8 x the largest entry of the reference block); c_k: rtol 1e-12 against the
    in-order sum"""
    for key in ("vx", "Vxx", "expected"):
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-7, atol=1e-8 * max(1.0, np.max(np.abs(ref[key]))), err_msg=f"{label} {key}")
    np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-12, atol=0.0, err_msg=f"{label} c")


# ---- the arithmetic of sddp_value_at_device, in float64 numpy in the stated order -----------------------------------------------
def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then one conversion)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def value_at_reference(c, expected, vx, Vxx, delta):
    """-> (the eight words but ok and node, i.e. value, lin, quad, c, expected, |delta|_inf) and the sum of the absolute values of the
    terms that enter `value` (the scale of its rounding error)"""
    nx = len(delta)
    t = np.zeros(nx)
    mag = abs(c) + abs(expected)
    for r in range(nx):
        acc = 0.0
        for j in range(nx):
            acc = fma(Vxx[r, j], delta[j], acc)
            mag += 0.5 * abs(Vxx[r, j] * delta[j] * delta[r])
        t[r] = acc
    lin = q2 = 0.0
    for r in range(nx):
        lin = fma(vx[r], delta[r], lin)
        mag += abs(vx[r] * delta[r])
    for r in range(nx):
        q2 = fma(delta[r], t[r], q2)
    quad = 0.5 * q2
    return np.array([((c + expected) + lin) + quad, lin, quad, c, expected, np.max(np.abs(delta))]), mag


# ---- the two experiments (check 6) ----------------------------------------------------------------------------------------------
# Instances and eps are those of the policy's first-order experiment (policy_cases.FO_CASES, fo_direction, FO_EPS, FO_OPTS).
# A converged solve at x0 gives the value record of node 0; J*(x0 + eps v) is the cost of the converged re-solve from x0 + eps v.
#
# lip30 is linear-quadratic: the model is exact, J*(x0 + eps v) == c_0 + expected_0 + lin + quad up to convergence and rounding.
# Measured on the oracle alone (tests/test_value_cpu.py): |J* - word 0| / c_0 = 5.456e-16 at eps = 4e-2 (J* = 8993.85) and 0.0 at
# eps = 1e-2 (J* = 6838.74), with c_0 = 6667.48: the rounding of the four-term sum.  LIP_ORACLE_ERROR is the larger of the two,
# rounded up in its second digit; the GPU test's bound is 100 x it.
LIP_ORACLE_ERROR = 5.5e-16
LIP_BOUND = 100.0 * LIP_ORACLE_ERROR
#
# srbd13: err(eps) = |J*(x0 + eps v) - c_0 - lin| falls like eps^2: err(eps) / err(eps / 4) > 8 (16 is the ideal), guarded against
# the convergence floor as policy_cases.assert_first_order guards its errors.  No third-order claim: the curvature is Gauss-Newton's.
# Measured on the oracle alone (c_0 = 97 861.5): err = 2.892e+03 at eps = 4e-2 and 1.823e+02 at eps = 1e-2, ratio 15.86.


def value_errors(model, c0, expected0, lin, quad, J_star):
    """per eps of FO_EPS: lin[i], quad[i] and J_star[i] = the re-solved cost -> the experiment's error per eps"""
    if model == "lip30":
        return [abs(J_star[i] - (((c0 + expected0) + lin[i]) + quad[i])) / abs(c0) for i in range(len(pc.FO_EPS))]
    return [abs(J_star[i] - c0 - lin[i]) for i in range(len(pc.FO_EPS))]


def assert_experiment(model, errs):
    e1, e2 = errs
    print(f"cost-to-go experiment {model}: err({pc.FO_EPS[0]}) = {e1:.3e}, err({pc.FO_EPS[1]}) = {e2:.3e}"
          + ("" if model == "lip30" else f", ratio {e1 / e2 if e2 else float('inf'):.2f}"))
    if model == "lip30":
        assert e1 <= LIP_BOUND and e2 <= LIP_BOUND, errs
    else:
        assert e2 > 1e-8, "errors at the convergence floor: the ratio would be noise"
        assert e1 / e2 > 8.0, errs
