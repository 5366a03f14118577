#!/usr/bin/env python3
"""A NON-LINEAR residual of your own on the reference's SRBD problem: what `prb.createResidual(name, expr)` with any CasADi
expression is upstream (python/prb.py:184-204; the reference's costs sum whatever the container holds, python/ddp.py:183-196).

    python examples/nonlinear_residual.py

The expression is written with sympy over `Variable.sym()` / `Parameter.sym()` and declared as a `problem.NonlinearTerm`; the
solver compiles it into a user build of the model (srbd_horizon_amd/userterms.py) -- once per problem shape: the gain and the
parameter values stay runtime data.  Here a leg-reach term keeps the distance from the CoM to the left-upper contact point at
most about the leg length `leg_len`: cost gain * (|c0 - r|^2 - leg_len^2)^2 on nodes 1..N.
Needs a GPU: the engine has no CPU fallback.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd.ddp import DDPSolver  # noqa: E402
from srbd_horizon_amd.prb import SRBDProblem  # noqa: E402
from srbd_horizon_amd.problem import NonlinearTerm  # noqa: E402

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)     # dsrbd_example.py:55-58


def build_problem(ns=20, T=1.0, leg_len=0.85):
    """The reference's srbd37 problem (prb.py:16-246, contact_model = 2) with the leg-reach term."""
    pb = SRBDProblem()
    prb = pb.createSRBDProblem(ns, T)
    var = {v.getName(): v for v in prb.var_container.getVarList(offset=False)}
    r, c0 = var["r"].sym(), pb.c[0].sym()                                 # sympy columns of the variables' entries
    L = prb.createParameter("leg_len", 1)                                 # a parameter of your own: per-node values
    L.assign(leg_len)
    e = (c0 - r).dot(c0 - r) - L.sym()[0] ** 2
    prb.createResidual("reach", NonlinearTerm(e, gain=1e3), nodes=range(1, ns + 1))
    return pb, prb


def main():
    ns = 20
    pb, prb = build_problem(ns)
    solver = DDPSolver(prb, OPTS)
    solver.setInitialState(pb.getInitialState())
    solver.set_u_warmstart(np.repeat(pb.getStaticInput()[:, None], ns, axis=1))
    ok = solver.solve()
    sol = solver.getSolutionDict()
    d = np.linalg.norm(sol["c0"] - sol["r"], axis=0)
    print(f"converged {ok} in {int(solver.stats['iters'])} iterations, cost {float(solver.stats['cost']):.4f}")
    print("|c0 - r| over the horizon:", np.round(d[::4], 4), " leg_len:", prb.getParameters()["leg_len"].values[0, 0])


if __name__ == "__main__":
    main()
