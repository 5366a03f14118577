#!/usr/bin/env python3
"""What one sddp_policy_covariance_device launch costs, next to the policy rollout over the same range and steps and the policy launch.

    python profiles/policy_covariance/measure.py

For srbd13 (N = 30) at B = 1024 and B = 20480 and srbd37 (N = 20) at B = 1024: workload.make_batch seeds 0 .. B - 1, all N knots of the
policy exported, one solve and its policy launch; then each of the three launches 2 times to warm up and 7 times timed with events on
the handle's stream (torch events on the stream the handle is bound to).  Sigma0 = 1e-4 I, q = r = NULL, all outputs given.  One JSON
line per case: median, min and max in ms of each."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from srbd_horizon_amd import _lib, workload  # noqa: E402

WARM, REPS = 2, 7


def timed(call):
    import torch
    for _ in range(WARM):
        call()
    t = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return dict(median=float(np.median(t)), min=min(t), max=max(t))


def main():
    import torch
    from srbd_horizon_amd.engine import DdpEngine
    for model, N, B in (("srbd13", 30, 1024), ("srbd13", 30, 20480), ("srbd37", 20, 1024)):
        batch = workload.make_batch(model, N, np.arange(B))
        eng = DdpEngine(model, N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), consts=batch["consts"])
        eng.use_torch_stream()
        eng.enable_policy(N)
        eng.load(batch["x0"], batch["xs"], batch["us"])
        x, _ = eng.solve(batch["params"])
        eng.policy_range_device()
        eng.synchronize()
        mk = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")      # noqa: E731
        s0 = (1e-4 * torch.eye(eng.nx, dtype=torch.float64, device="cuda")).repeat(B, 1, 1).contiguous()
        out, cov, ud = mk(B, _lib.POLICY_COV_WORDS), mk(B, N + 1, eng.nx, eng.nx), mk(B, N, eng.nu)
        xm, xr, ur = torch.from_numpy(np.ascontiguousarray(x[:, 0])).cuda(), mk(B, N + 1, eng.nx), mk(B, N, eng.nu)
        res = dict(model=model, N=N, B=B, steps=N, warmup=WARM, reps=REPS,
                   covariance_ms=timed(lambda: eng.policy_covariance_device(s0, out, None, None, cov, ud)),
                   covariance_record_only_ms=timed(lambda: eng.policy_covariance_device(s0, out)),
                   rollout_ms=timed(lambda: eng.policy_rollout_device(xm, xr, ur)),
                   policy_launch_ms=timed(lambda: eng.policy_range_device()))
        print(json.dumps(res), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
