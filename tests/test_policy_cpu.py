"""Policy export, what needs no GPU: the record layout arithmetic, the FleetQueue's mode-2 ("first_knot_policy") record at world
size 2 on gloo with the engine stand-in of tests/test_fleet_gloo.py, MpcLoop's default path, and the oracle-only run of the
first-order experiment that tests/test_gpu_policy.py repeats on the device (instances and eps are chosen HERE, on the oracle)."""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import ddp as oddp, models as omodels
from srbd_horizon_amd import dist as sdist, workload
from srbd_horizon_amd.fleet import FleetQueue
from tests import abi_header, policy_cases as pc
from tests.fleet_support import N, NP, NU, NX, OPTS, OracleEngine, free_port as _free_port, seeds_of as _seeds


def test_policy_record_layout_arithmetic():
    """words = knots * nu * (nx + 1) + 4 (sddp_policy_words); the mode-2 record is the first-knot record plus nu * (nx + 1)"""
    assert "words = knots * nu * (nx + 1) + 4" in open(abi_header.HEADER).read()      # the header's own statement of it, a comment
    for (n, nx, nu) in ((30, 13, 6), (20, 37, 24), (20, 30, 15), (20, 61, 48)):
        first = sdist.record_words(n, nx, nu, "first_knot")
        assert first == nu + nx + 2
        assert sdist.record_words(n, nx, nu, "first_knot_policy") == first + nu * (nx + 1)
        assert sdist.record_words(n, nx, nu, "full") == (n + 1) * nx + n * nu + 2
    assert sdist.record_words(30, 13, 6, "first_knot_policy") == 21 + 84
    from srbd_horizon_amd.engine import DdpEngine
    assert DdpEngine.RECORD_MODES == {"full": 0, "first_knot": 1, "first_knot_policy": 2}
    # split_policy: the record's layout, without a handle
    nu, nx, M = 6, 13, 3
    rec = np.arange(2 * (M * nu * (nx + 1) + 4), dtype=float).reshape(2, -1)
    eng = DdpEngine.__new__(DdpEngine)
    eng.nu, eng.nx = nu, nx
    kff, K, info = DdpEngine.split_policy(eng, rec)
    assert kff.shape == (2, M, nu) and K.shape == (2, M, nu, nx) and info.shape == (2, 4)
    w = nu * (nx + 1)
    np.testing.assert_array_equal(kff[1, 2], rec[1, 2 * w:2 * w + nu])
    np.testing.assert_array_equal(K[1, 2, 4], rec[1, 2 * w + nu + 4 * nx:2 * w + nu + 5 * nx])
    np.testing.assert_array_equal(info[0], rec[0, -4:])
    eng.h = None


class PolicyOracleEngine(OracleEngine):
    """the stand-in with the policy surface: policy_range_device fills `policy_records` [B, nu (nx + 1) + 4] with the numpy oracle"""

    def __init__(self, B):
        super().__init__(B)
        self.policy_records = torch.zeros(B, NU * (NX + 1) + 4, dtype=torch.float64)
        self._P = None

    def solve_range_device(self, params, first, count):
        super().solve_range_device(params, first, count)
        self._P = params

    def policy_range_device(self, first, count):
        m = omodels.make_model("srbd13")
        opt = oddp.DdpOptions(**OPTS)
        for b in range(first, first + count):
            # (the C oracle's record keeps cost and iterations only: a converged solve ends with closed gaps, mu0 and a full step)
            st = dict(gap=0.0, mu=opt.mu0, alpha=opt.alpha_0, status=0)
            kff, K, info = pc.oracle_policy(m, self.x[b].numpy(), self.u[b].numpy(), self._P[b].numpy(), st, opt, 1)
            self.policy_records[b] = torch.from_numpy(np.concatenate([kff[0], K[0].reshape(-1), info]))


def _worker(rank, world, port, B, depth, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    P0 = torch.zeros(depth * B, N + 1, NP, dtype=torch.float64)
    eng = PolicyOracleEngine(depth * B)
    fleet = FleetQueue(eng, P0, B, depth, collective=True, gather="first_knot", policy=True)
    for s in range(depth):
        batch = workload.make_batch("srbd13", N, _seeds(rank, depth, s, B))
        t = {k: torch.from_numpy(batch[k]) for k in ("x0", "xs", "us", "params")}
        fleet.submit(t["x0"], t["xs"], t["us"], t["params"])
    fleet.flush()
    fleet.wait()
    q.put((rank, fleet.gather_bytes, fleet.gathered.numpy().copy(), eng.x.numpy().copy(), eng.u.numpy().copy(),
           eng.policy_records.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_fleet_mode2_records_world2():
    world, B, depth = 2, 2, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, B, depth, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    W = sdist.record_words(N, NX, NU, "first_knot_policy")
    assert W == NU + NX + 2 + NU * (NX + 1) == 105
    n = B * depth
    for rank, gbytes, rec, x, u, pol in res:
        assert gbytes == n * W * 8
        assert rec.shape == (world * n, W)
        np.testing.assert_array_equal(rec, res[0][2])                         # every rank ends with the same gathered tensor
        mine = rec[rank * n:(rank + 1) * n]
        np.testing.assert_array_equal(mine[:, :NU], u[:, 0])
        np.testing.assert_array_equal(mine[:, NU:NU + NX], x[:, 1])
        np.testing.assert_array_equal(mine[:, NU + NX + 2:], pol[:, :NU * (NX + 1)])      # kff_0 | K_0 behind the mode-1 record
        assert np.all(pol[:, -1] == 1.0) and np.max(np.abs(mine[:, NU + NX + 2 + NU:])) > 0.0
    with pytest.raises(ValueError):
        FleetQueue(OracleEngine(4), torch.zeros(4, N + 1, NP, dtype=torch.float64), 2, 2, gather="full", policy=True)


def test_mpc_loop_default_is_the_open_loop_path():
    """feedback_substeps defaults to 0 and the default tick never touches the policy calls (no GPU: read from the source)"""
    from srbd_horizon_amd.mpc import MpcLoop
    sig = inspect.signature(MpcLoop.__init__)
    assert sig.parameters["feedback_substeps"].default == 0 and sig.parameters["feedback"].default is True
    assert inspect.signature(MpcLoop.tick).parameters["push"].default is None
    src = inspect.getsource(MpcLoop.tick)
    assert "if self.feedback_substeps > 0:" in src and "get_feedback_gains" not in src
    assert "get_feedback_gains" in inspect.getsource(MpcLoop._substeps)


@pytest.mark.parametrize("model", ["lip30", "srbd13"])
def test_first_order_property_in_the_oracle(model):
    """Check 5 on the numpy oracle alone, with the instances and eps of tests/policy_cases.py (second_order = 1, the default).
    Measured: srbd13 err 1.48e-3 / 8.94e-5, ratio 16.5 (at eps / 16: 9.8e-6, ratio 9.1 -- the part of the Hessian that
    second_order = 1 leaves out begins to show; second_order = 2 gives 15.9 and 16.0); lip30 3.6e-15 at both (exact)."""
    n, seed = pc.FO_CASES[model]
    b = workload.make_batch(model, n, [seed])
    m = omodels.make_model(model, omodels.RobotConsts(**b["consts"]))
    opt = oddp.DdpOptions(**pc.FO_OPTS)
    x0, P = b["x0"][0], b["params"][0]
    r = oddp.solve(m, x0, P, b["xs"][0], b["us"][0], opt)
    assert r.converged
    _, K, info = pc.oracle_policy(m, r.xs, r.us, P, dict(gap=r.gap, mu=r.mu, alpha=r.alpha, status=r.status), opt, 1)
    assert info[3] == 1.0 and info[1] == (1.0 if model != "lip30" or r.alpha == 1.0 else 0.0)
    v = pc.fo_direction(model, m.nx)

    def resolve(eps):
        xs = r.xs.copy()
        r2 = oddp.solve(m, x0 + eps * v, P, xs, r.us, opt)
        assert r2.converged
        return r2.us[0]

    pc.assert_first_order(model, pc.fo_errors(r.us[0], K[0], v, resolve))
