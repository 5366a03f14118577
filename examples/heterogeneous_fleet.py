#!/usr/bin/env python3
"""A heterogeneous fleet in ONE handle: robots that carry different payloads (include/sddp.h: sddp_set_instance_consts).

    python examples/heterogeneous_fleet.py [--robots 1024] [--blocks 4] [--horizon 30]

`--robots` cold-started srbd13 MPC instances carry a payload of 0 - 25 % of the body mass (mass and inertia scaled with it) and
live in one handle, one queue, one launch: every kernel reads instance b's own constants.  Prints the iterations by payload
quartile, and the same fleet solved as if every robot were the bare one.  Needs a GPU: the engine has no CPU fallback.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402
from srbd_horizon_amd.fleet import FleetQueue  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--horizon", type=int, default=30)
    args = ap.parse_args()
    B, N, R = args.robots // args.blocks, args.horizon, args.robots // args.blocks * args.blocks
    dev = torch.device("cuda", 0)
    opts = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3, waves_per_simd=2, queue_order=2)
    eng = DdpEngine("srbd13", N, R, opts=opts)
    blocks = []
    for k in range(args.blocks):
        b = workload.make_batch("srbd13", N, k * B + np.arange(B))
        blocks.append({n: torch.from_numpy(b[n]).to(dev) for n in ("x0", "xs", "us", "params")})
    fleet = FleetQueue(eng, torch.cat([b["params"] for b in blocks]).contiguous(), B, args.blocks)

    def tick():
        for b in blocks:
            fleet.submit(b["x0"], b["xs"], b["us"])
        fleet.flush()
        return eng.fetch()[2]

    bare = tick()                                                    # every robot the handle's own: no payload
    payload = np.random.default_rng(0).uniform(0.0, 0.25, R)         # fraction of the body mass
    I0 = np.asarray(list(eng.consts.I)).reshape(3, 3)
    fleet.set_instance_consts({"m": eng.consts.m * (1.0 + payload), "I": I0[None] * (1.0 + payload)[:, None, None]})
    st = tick()
    slots, grid, queued = eng.queue_info()
    print(f"{R} robots, payload 0 - 25 % of {eng.consts.m:.0f} kg, one launch: "
          + (f"queue of {queued} on {grid} slots" if queued else f"{grid} resident slots, one per robot (more robots than slots queue)"))
    edges = np.quantile(payload, [0.0, 0.25, 0.5, 0.75, 1.0])
    for q in range(4):
        sel = (payload >= edges[q]) & ((payload < edges[q + 1]) | (q == 3))
        print(f"  payload {100 * edges[q]:4.1f} - {100 * edges[q + 1]:4.1f} %: iterations mean {st['iters'][sel].mean():5.1f} max {st['iters'][sel].max():3d} "
              f"| converged {st['converged'][sel].mean():.3f} | the same robots without payload: mean {bare['iters'][sel].mean():5.1f}")
    print(f"  {int((st['iters'] != bare['iters']).sum())} of {R} robots take another iteration count than the bare robot")


if __name__ == "__main__":
    main()
