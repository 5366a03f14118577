"""What the policy-rollout tests share (tests/test_policy_rollout_cpu.py, tests/test_gpu_policy_rollout.py): the rule of
sddp_policy_rollout_device, stated once in numpy over the oracle's model, and the one-step check the GPU test makes with it.

THE RULE.  From a measured state at node `start`, with the plan (xs, us), the parameters P and the exported gains K of one instance:
    x_0' = x_meas;   u_j' = us[k] + K[k] (x_j' - xs[k]);   x_{j+1}' = f(x_j', u_j', P[k]);   k = start + j,   j = 0 .. steps - 1
    cost = sum_j L_k(x_j', u_j'), added in knot order
f and L are the model's own (oracle.models.Model.f / .cost): no quaternion renormalisation, no sub-stepping.  ok = 0 (the policy
record's last word): K is not multiplied at all -- whatever it holds -- and the rollout is the open-loop one of us[k].
"""
import numpy as np


def rollout_reference(m, xs, us, P, K, ok, x_meas, start, steps):
    """one instance -> (x [steps + 1, nx], u [steps, nu], cost); K [>= start + steps, nu, nx]"""
    x = np.empty((steps + 1, m.nx))
    u = np.empty((steps, m.nu))
    x[0] = x_meas
    cost = 0.0
    for j in range(steps):
        k = start + j
        u[j] = us[k] + K[k] @ (x[j] - xs[k]) if ok else us[k]
        cost += m.cost(x[j], u[j], P[k], k)
        x[j + 1] = m.f(x[j], u[j], P[k])
    return x, u, cost


def assert_rollout_shadows(m, xs, us, P, K, ok, start, got_x, got_u, got_cost, label=""):
    """One instance's device rollout (got_x [steps + 1, nx], got_u [steps, nu], got_cost) against the rule, knot by knot FROM THE
    DEVICE'S OWN x_j', so nothing compounds over the knots.  Every bound is one an existing test gives the same quantity:
      input: |u_j' - (us_k + K_k (x_j' - xs_k))| <= 1e-12 max|K_k| max|x_j' - xs_k| nx, absolute (test_apply_policy_device);
      state: x_{j+1}' against m.f(x_j', u_j', P_k) at rtol 1e-12 (the model_step parity tests);
      cost:  got_cost against sum_j m.cost(x_j', u_j', P_k, k) at rtol 1e-11 (the knot level of test_eval_knots_matches_oracle;
             the terms are sums of squares, so the sum loses nothing).
    -> the worst (input error / its bound, relative state error, relative cost error), for printing."""
    steps = got_u.shape[0]
    assert got_x.shape == (steps + 1, m.nx) and got_u.shape == (steps, m.nu), (label, got_x.shape, got_u.shape)
    cost = 0.0
    worst_u = worst_x = 0.0
    for j in range(steps):
        k = start + j
        dx = got_x[j] - xs[k]
        if ok:
            ref_u = us[k] + K[k] @ dx
            bound = 1e-12 * np.max(np.abs(K[k])) * np.max(np.abs(dx)) * m.nx
        else:
            ref_u, bound = us[k], 0.0
        err = float(np.max(np.abs(got_u[j] - ref_u)))
        worst_u = max(worst_u, err / bound if bound > 0.0 else (0.0 if err == 0.0 else np.inf))
        assert err <= bound, f"{label} knot {k}: input error {err:.3e} > {bound:.3e}"
        fo = m.f(got_x[j], got_u[j], P[k])
        worst_x = max(worst_x, float(np.max(np.abs(got_x[j + 1] - fo) / np.maximum(np.abs(fo), 1e-300))))
        np.testing.assert_allclose(got_x[j + 1], fo, rtol=1e-12, atol=0.0, err_msg=f"{label} knot {k}: state")
        cost += m.cost(got_x[j], got_u[j], P[k], k)
    np.testing.assert_allclose(got_cost, cost, rtol=1e-11, atol=0.0, err_msg=f"{label}: cost")
    return worst_u, worst_x, abs(float(got_cost) - cost) / abs(cost)
