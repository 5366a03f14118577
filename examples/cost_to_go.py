#!/usr/bin/env python3
"""What a push costs each robot of a fleet, predicted from the previous plan's value function and checked by re-solving.

    python examples/cost_to_go.py [--robots 1024] [--push 0.2] [--top 128]

`--robots` srbd13 robots are solved once (N = 30) with the value function of node 0 exported (sddp_enable_value: the quadratic model
c_0 + expected_0 + vx_0 . d + 1/2 d^T Vxx_0 d that the policy's backward sweep holds).  Every robot is then pushed as in
policy_rollout.py, each with its own strength: its measured state is x_0 + delta, delta a lateral CoM velocity of up to `--push` m/s.
sddp_value_at_device predicts the cost of the best plan from there; the fleet is then re-solved from the pushed states to convergence.
Prints the rank correlation between the predicted cost increase (word 0 - c_0) and the actual one (re-solved cost - c_0), and the
share of the `--top` most affected robots that the prediction also ranks in its top `--top`: the list a server would re-solve first
under a time budget.  The model's second order is the sweep's Gauss-Newton one: a ranking tool, not the Hessian of the optimal cost.
Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402


def ranks(a):
    r = np.empty(len(a))
    r[np.argsort(a, kind="stable")] = np.arange(len(a))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--push", type=float, default=0.2)
    ap.add_argument("--top", type=int, default=128)
    a = ap.parse_args()
    N, B, top = 30, a.robots, min(a.top, a.robots)
    batch = workload.make_batch("srbd13", N, np.arange(B))
    opts = dict(max_iters=200, alpha_converge_threshold=1e-12, beta=1e-3)
    eng = DdpEngine("srbd13", N, B, opts=opts, consts=batch["consts"])
    eng.enable_policy(1)
    eng.enable_value(1)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    eng.policy_range_device()                                    # one sweep per robot: gains and value records in the same launch
    x_meas = x[:, 0].copy()
    x_meas[:, 8] += a.push * np.random.default_rng(0).uniform(-1.0, 1.0, B)      # x = r | o | rdot | w: the lateral CoM velocity
    rec = eng.value_at(x_meas, node=0)
    ok = rec[:, 6] == 1.0
    predicted = rec[:, 0] - rec[:, 3]
    eng.load(x_meas, x, u)                                       # the converged re-solve from the pushed states
    eng.solve(batch["params"])
    ok &= eng.stats["converged"] == 1
    actual = eng.stats["cost"] - rec[:, 3]
    eng.close()
    p, q = predicted[ok], actual[ok]
    rho = np.corrcoef(ranks(p), ranks(q))[0, 1]
    k = min(top, len(p))
    hit = len(set(np.argsort(-p)[:k]) & set(np.argsort(-q)[:k])) / max(k, 1)
    print(f"{int(ok.sum())} of {B} robots with a policy and a converged re-solve")
    print(f"cost increase after the push: predicted median {np.median(p):.4g}, actual median {np.median(q):.4g}; "
          f"median |predicted - actual| / actual {np.median(np.abs(p - q) / np.maximum(np.abs(q), 1e-300)):.3g}")
    print(f"rank correlation (Spearman) of predicted and actual increase: {rho:.4f}")
    print(f"of the {k} most affected robots, the prediction ranks {100.0 * hit:.1f} % in its own top {k}")


if __name__ == "__main__":
    main()
