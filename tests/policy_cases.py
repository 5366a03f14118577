"""What the policy-export tests share (tests/test_policy_cpu.py, tests/test_gpu_policy.py): the rule of the exported sweep, stated
here in the tests' own words and evaluated with the numpy oracle, and the first-order experiment.

THE RULE.  The policy of an instance is ONE backward sweep at the trajectory (xs, us) a solve returned, made with what the
iteration would carry into its next sweep:
  * defects: those of the returned trajectory, d_k = f(x_k, u_k) - x_{k+1}; exact zeros once the gaps count as closed
    (the solve's remaining defect norm <= gap_tol);
  * regularisation: the solve's final mu; if a Quu is not positive definite, first the second-order term is dropped, then
    mu <- 10 max(mu, 0) + mu_min until the sweep passes, giving up above mu_max (ok = 0, all gains zero);
  * second-order term: on (theta = 1) iff the options ask for it and the solve's last step length was the full one, alpha_0.
An iterate the solve refused for its non-finite cost (status 3) has no policy: no sweep, ok = 0, all gains zero, mu_used = the
solve's mu.  (A Quu that does not depend on the non-finite entry would otherwise pass the sweep and carry the NaN into the gains.)
The record per instance: kff_k, K_k for the first M knots, then mu_used, theta_used, expected = -(dV1 + dV2), ok.
"""
import numpy as np

from oracle import ddp as oddp


def oracle_policy(m, xs, us, P, stats, opt: oddp.DdpOptions, knots: int):
    """-> kff [M, nu], K [M, nu, nx], info [4] by the rule above; stats: the solve's record (alpha, gap, mu, status)"""
    N = us.shape[0]
    M = min(knots, N)
    if int(stats["status"]) == 3:
        return np.zeros((M, m.nu)), np.zeros((M, m.nu, m.nx)), np.array([float(stats["mu"]), 0.0, 0.0, 0.0])
    d = oddp.defects(m, xs, us, P) if float(stats["gap"]) > opt.gap_tol else np.zeros((N, m.nx))
    mu = float(stats["mu"])
    theta = 1.0 if (opt.second_order and float(stats["alpha"]) == opt.alpha_0) else 0.0
    while True:
        ok, K, kff, dV1, dV2 = oddp.backward_pass(m, xs, us, P, d, mu, theta, int(opt.second_order) or 1)[:5]
        if ok:
            return kff[:M].copy(), K[:M].copy(), np.array([mu, theta, -(dV1 + dV2), 1.0])
        if theta:
            theta = 0.0
            continue
        mu = max(mu, 0.0) * 10.0 + opt.mu_min
        if mu > opt.mu_max:
            return np.zeros((M, m.nu)), np.zeros((M, m.nu, m.nx)), np.array([mu, theta, 0.0, 0.0])


def assert_policy_matches(kff, K, info, ref, label=""):
    """one instance against oracle_policy's result, at the tolerance the project uses for one backward sweep
    (tests/test_gpu_parity.py: rtol 1e-7, atol 1e-8 x the largest entry)"""
    ko, Ko, io = ref
    np.testing.assert_allclose(K, Ko, rtol=1e-7, atol=1e-8 * max(1.0, np.max(np.abs(Ko))), err_msg=label)
    np.testing.assert_allclose(kff, ko, rtol=1e-7, atol=1e-8 * max(1.0, np.max(np.abs(ko))), err_msg=label)
    assert info[0] == io[0] and info[1] == io[1] and info[3] == io[3], (label, info, io)          # mu_used, theta_used, ok: exact
    assert abs(info[2] - io[2]) <= 1e-8 * max(1.0, abs(io[2])), (label, info, io)                  # expected


# ---- the first-order experiment (check 5 of the policy export) ----------------------------------------------------------------
# A converged solve at x0 gives u_0 and the policy's K_0; the optimal first input of the problem started at x0 + eps v is
# u_0 + K_0 eps v + O(eps^2) IF K_0 is the derivative of the optimal first input.  Tight options: the convergence floor of u_0
# (~1e-11) has to sit well below the errors compared (1.5e-3 and 9e-5 for srbd13 at these eps).
FO_OPTS = dict(max_iters=200, alpha_converge_threshold=1e-12, beta=1e-3, cost_reduction_ths=1e-14)
FO_EPS = (4e-2, 1e-2)                           # eps and eps / 4
FO_CASES = {"srbd13": (30, 0), "lip30": (20, 5)}          # model -> (N, workload seed)


def fo_direction(model, nx, seed=1):
    v = np.random.default_rng(seed).standard_normal(nx)
    if model != "lip30":
        v[3:7] = 0.0                            # stay on the unit quaternion
    return v / np.linalg.norm(v)


def fo_errors(u0, K0, v, resolve):
    """resolve(eps) -> first input of the converged solve from x0 + eps v.  -> [(error, size of the linear term)] per FO_EPS"""
    out = []
    for eps in FO_EPS:
        out.append((float(np.max(np.abs(resolve(eps) - (u0 + K0 @ (eps * v))))), float(np.max(np.abs(K0 @ (eps * v))))))
    return out


def assert_first_order(model, errs):
    """The error of the policy's prediction falls like eps^2: err(eps) / err(eps / 4) > 8 (16 is the ideal).
    lip30 is linear-quadratic: its optimal first input is EXACTLY affine in x0, the error is rounding (measured 3.6e-15 against a
    linear term of 1.4 and 0.35, oracle and GPU alike) and the ratio of two rounding errors says nothing (1.0 in the oracle).
    There the assertion is the stronger statement the decay law tends to: both errors below 1e-12 x the linear term."""
    (e1, l1), (e2, l2) = errs
    print(f"first-order check {model}: err({FO_EPS[0]}) = {e1:.3e} (linear term {l1:.3e}), err({FO_EPS[1]}) = {e2:.3e} "
          f"(linear term {l2:.3e}), ratio {e1 / e2 if e2 else float('inf'):.2f}")
    if model == "lip30":
        assert e1 <= 1e-12 * l1 and e2 <= 1e-12 * l2, errs
    else:
        assert e2 > 1e-8, "errors at the convergence floor: the ratio would be noise"
        assert e1 / e2 > 8.0, errs
