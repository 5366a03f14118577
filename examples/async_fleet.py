#!/usr/bin/env python3
"""A fleet whose robots re-plan at different rates, in ONE resident handle: masked advance, masked solve, masked policy export.

    python examples/async_fleet.py [--robots 1024] [--ticks 12] [--threshold 0.05] [--push 0.3]

`--robots` srbd13 robots (N = 30) live in one handle with resident parameters.  A third of them re-plans every tick, a third every
second and a third every fourth tick, with staggered phases.  A tick is one knot of time: every robot's age (knots since its last
re-plan) grows by one, and its measured state is the state its plan expects at that node plus noise -- and, for a random 5 % of
the fleet per tick, a lateral push of `--push` m/s on the CoM velocity.  Per tick, all on the device and with no host synchronisation
before the launches:
  * sddp_value_at_device predicts, from the value records of every robot's last policy sweep, what its measured state costs;
  * the mask is every robot that is DUE (age = its period) plus every robot whose predicted cost increase exceeds `--threshold`
    times the cost-to-go of its plan at that node (the stated threshold: 5 % by default);
  * sddp_advance_masked_device shifts the selected robots by their age (one launch per knot, at most four) and sets their measured
    state, sddp_solve_masked_device re-solves them on the resident parameters, sddp_policy_masked_device renews their policy and
    value records.  Every other robot keeps its plan, its records and its age.
The new last parameter row of an advanced robot repeats its previous last row (a frozen schedule: the example is about the launch
sequence, examples/mpc_loop.py has a gait generator).  Prints, per tick, how many robots were due, how many the threshold added, how
many were solved (sddp_last_selected) and the time of the tick's launch sequence between two events on the handle's stream.
Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import _lib, workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402

PERIODS = (1, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--push", type=float, default=0.3)
    a = ap.parse_args()
    model, N, B, top = "srbd13", 30, a.robots, max(PERIODS)
    batch = workload.make_batch(model, N, np.arange(B))
    eng = DdpEngine(model, N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), consts=batch["consts"])
    eng.use_torch_stream()
    eng.enable_policy(1)
    eng.enable_value(top + 1)                                    # the value function of the nodes 0 .. 4: a robot is at most 4 knots old
    eng.set_params(batch["params"])
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve_resident()
    eng.policy_range_device()
    P = eng.device_view(_lib.BUF_PARAMS, (B, N + 1, eng.np_))    # zero-copy views, ordered on the stream the handle shares with torch
    xs = eng.device_view(_lib.BUF_XS, (B, N + 1, eng.nx))
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = torch.arange(B, device="cuda")
    period = torch.tensor(PERIODS, device="cuda")[rows % len(PERIODS)]
    age = (rows // len(PERIODS)) % period                        # staggered phases
    rec = torch.empty((top + 1, B, _lib.VALUE_AT_WORDS), dtype=torch.float64, device="cuda")
    print(f"{B} robots, periods {PERIODS}, threshold {a.threshold:g} of the plan's cost-to-go, push {a.push:g} m/s on 5 % per tick")
    print("tick   due  +threshold  solved  not converged  launch sequence ms")
    for tick in range(a.ticks):
        age = age + 1
        x_meas = xs[rows, age] + 1e-3 * torch.randn((B, eng.nx), generator=gen, dtype=torch.float64, device="cuda")
        pushed = torch.rand(B, generator=gen, device="cuda") < 0.05
        x_meas[:, 8] += a.push * pushed                          # x = r | o | rdot | w: the lateral CoM velocity
        x_meas = x_meas.contiguous()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for node in range(1, top + 1):                           # the prediction at every age a robot can have; each robot reads its own
            eng.value_at_device(x_meas, rec[node], node)
        mine = rec[age, rows]
        increase, c_k, ok = mine[:, 0] - mine[:, 3], mine[:, 3], mine[:, 6] == 1.0
        due = age >= period
        alarm = ok & ~due & (increase > a.threshold * c_k.abs())
        select = due | alarm
        p_last = P[:, N].clone()
        for j in range(top):                                     # one knot per launch: a robot advances by its age
            eng.advance_masked_device((select & (age > j)).to(torch.int32), p_last, x_meas)
        mask = select.to(torch.int32)
        eng.solve_masked_device(None, mask)
        eng.policy_masked_device(mask)
        t1.record()
        age = torch.where(select, torch.zeros_like(age), age)
        t1.synchronize()
        st = eng.fetch()[2]
        bad = int(np.count_nonzero((st["converged"] != 1) & select.cpu().numpy()))
        print(f"{tick:4d}  {int(due.sum()):4d}  {int(alarm.sum()):10d}  {eng.last_selected():6d}  {bad:13d}  {t0.elapsed_time(t1):18.3f}")
    eng.close()


if __name__ == "__main__":
    main()
