"""The CPU stand-in for the engine behind fleet.FleetQueue, and the bookkeeping of a world-size-2 gloo run, shared by
tests/test_fleet_gloo.py and tests/test_policy_cpu.py."""
import socket

import numpy as np
import torch

from oracle import cport
from srbd_horizon_amd import _lib
from tests import oracle_refs as refs

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)
N, NX, NU, NP = 30, 13, 6, 19


class OracleEngine:
    """CPU stand-in with the engine's queue surface (load_range_device / solve_range_device / fetch_device_views)."""

    def __init__(self, B):
        self.B = B
        self.x0 = torch.zeros(B, NX, dtype=torch.float64)
        self.x = torch.zeros(B, N + 1, NX, dtype=torch.float64)
        self.u = torch.zeros(B, N, NU, dtype=torch.float64)
        self.stats = np.zeros(B, dtype=_lib.STATS_DTYPE)
        self.sf = torch.from_numpy(self.stats.view(np.float64).reshape(B, _lib.STATS_F64_WORDS))
        self.si = torch.from_numpy(self.stats.view(np.int32).reshape(B, _lib.STATS_I32_WORDS))

    def load_range_device(self, first, count, x0=None, x=None, u=None):
        s = slice(first, first + count)
        if x0 is not None: self.x0[s] = x0
        if x is not None: self.x[s] = x
        if u is not None: self.u[s] = u

    def solve_range_device(self, params, first, count):
        s = slice(first, first + count)
        start = dict(x0=self.x0[s].numpy(), params=params[s].numpy(), xs=self.x[s].numpy(), us=self.u[s].numpy(), consts={})      # the default robot
        xo, uo, so = refs.c_oracle("srbd13", start, OPTS, threads=2)
        self.x[s] = torch.from_numpy(xo.copy())
        self.u[s] = torch.from_numpy(uo.copy())
        self.stats["cost"][s] = cport.stat(so, "cost")
        self.stats["iters"][s] = cport.stat(so, "iters").astype(np.int32)

    def fetch_device_views(self):
        return self.x, self.u, self.sf, self.si


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def seeds_of(rank, steps, step, B):
    return (rank * steps + step) * B + np.arange(B)                    # bench.py: every step of every rank solves its own instances
