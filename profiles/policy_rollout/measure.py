#!/usr/bin/env python3
"""The policy rollout's two mappings, timed on one solved fleet: one wavefront per instance (the library's policy_rollout_kernel)
against one lane per instance (the mapping of model_step_kernel, kept in measure.hip only).

    python profiles/policy_rollout/measure.py [--build-only] [--robots 1024] [--steps 4] [--reps 200]

srbd13, N = 30, workload.make_batch seeds 0..robots-1, enable_policy(steps), one solve and its policy launch; every robot's measured
state is x_0 + 1e-2 randn.  Prints one JSON line: the best and mean HIP-event time of each kernel over `--reps` launches after three
warm-up launches, whether the two mappings gave the same bytes, and, through the engine on the handle's stream, the time of
sddp_policy_rollout_device and of sddp_apply_policy_knot_device.  The comparison library is compiled into build/ by the compile
command of the model builds (--build-only: just that, where there is a compiler and no GPU)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from srbd_horizon_amd import _lib, workload  # noqa: E402

LIB = os.path.join(ROOT, "build", "policy_rollout_measure.so")


def build():
    src = os.path.join(HERE, "measure.hip")
    if not (os.path.exists(LIB) and os.path.getmtime(LIB) >= max(os.path.getmtime(p) for p in [src] + [os.path.join(_lib.CSRC, h) for h in _lib.HEADERS])):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.run(_lib.compile_command() + ["-shared", src, "-o", LIB], check=True)
    return LIB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    build()
    if a.build_only:
        return
    import torch
    from srbd_horizon_amd.engine import DdpEngine
    N, B, M = 30, a.robots, a.steps
    batch = workload.make_batch("srbd13", N, np.arange(B))
    eng = DdpEngine("srbd13", N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), consts=batch["consts"])
    eng.enable_policy(M)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, _ = eng.solve(batch["params"])
    eng.policy_range_device()
    eng.synchronize()
    xm = torch.from_numpy(x[:, 0] + 1e-2 * np.random.default_rng(0).standard_normal((B, eng.nx))).cuda()
    out = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((B, M + 1, eng.nx), (B, M, eng.nu), (B,)) * 2]
    lib = C.CDLL(LIB)
    ms = (C.c_float * 4)()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    torch.cuda.synchronize()
    rc = lib.measure_rollouts(C.byref(eng.consts), N, B, 0, M, *(C.c_void_p(eng.device_buffer(w)[0]) for w in (0, 1, 5, 8)), eng.policy_words()[0],
                              p(xm), *(p(t) for t in out), a.reps, ms)
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = dict(model="srbd13", N=N, count=B, steps=M, reps=a.reps, wave_best_us=1e3 * ms[0], wave_mean_us=1e3 * ms[1], lane_best_us=1e3 * ms[2],
               lane_mean_us=1e3 * ms[3], same_bytes=all(torch.equal(out[i], out[i + 3]) for i in range(3)),
               max_abs_diff_x=float((out[0] - out[3]).abs().max()))
    # through the library's entry points, on the handle's stream (torch events on that stream)
    eng.use_torch_stream()
    u1 = torch.empty((B, eng.nu), dtype=torch.float64, device="cuda")
    for name, call in (("rollout_api_us", lambda: eng.policy_rollout_device(xm, out[0], out[1], out[2])),
                       ("apply_knot_api_us", lambda: eng.apply_policy_device(xm, u1, knot=M - 1))):
        for _ in range(3):
            call()
        t = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            e1.synchronize()
            t.append(1e3 * e0.elapsed_time(e1))
        res[name + "_best"], res[name + "_mean"] = min(t), float(np.mean(t))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
