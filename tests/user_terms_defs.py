"""Problems with user residuals that the user-term tests solve (tests/test_user_terms.py, tests/test_gpu_user_terms.py) and the
example's, in one place: ``__graft_entry__.build()`` pre-builds their user builds with ``prebuild()`` so that a tree built on one
machine runs them on another without a compiler."""
from __future__ import annotations

import importlib.util
import os

import numpy as np

from srbd_horizon_amd import userterms
from srbd_horizon_amd.prb import SRBD13Problem
from srbd_horizon_amd.problem import LinearTerm, NonlinearTerm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def example_module():
    spec = importlib.util.spec_from_file_location("nonlinear_residual_example", os.path.join(ROOT, "examples", "nonlinear_residual.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _var(prb):
    return {v.getName(): v for v in prb.var_container.getVarList(offset=False)}


def srbd13_terrain(ns, a=0.03, k=6.0, h0=0.85, gain=1e3):
    """srbd13 with a terrain-height term r_z - h0 - a sin(k r_x) on nodes 1..N (a, k, h0: parameters of the user's)."""
    pb = SRBD13Problem()
    prb = pb.createSRBD13Problem(ns, 1.0)
    r = _var(prb)["r"].sym()
    ter = prb.createParameter("terrain", 3)                  # a, k, h0
    ter.assign(np.array([a, k, h0]))
    import sympy
    t = ter.sym()
    prb.createResidual("terrain", NonlinearTerm(r[2] - t[2] - t[0] * sympy.sin(t[1] * r[0]), gain=gain), nodes=range(1, ns + 1))
    return pb, prb


# the same two rows declared as LinearTerm (the _x build) or as NonlinearTerm (a user build): a state row rdot_x + 0.2 r_x - ref
# (ref: a parameter) and a stage row f0_z - f1_z
PAIR_GAINS = (3e2, 1e-3)


def srbd13_pair(ns, nonlinear: bool):
    pb = SRBD13Problem()
    prb = pb.createSRBD13Problem(ns, 1.0)
    v = _var(prb)
    ref = prb.createParameter("vx_ref", 1)
    ref.assign(np.linspace(0.0, 0.3, ns + 1)[None])
    if nonlinear:
        r, rd, f0, f1 = v["r"].sym(), v["rdot"].sym(), v["f0"].sym(), v["f1"].sym()
        prb.createResidual("vx", NonlinearTerm(rd[0] + 0.2 * r[0] - ref.sym()[0], gain=PAIR_GAINS[0]), nodes=range(1, ns + 1))
        prb.createResidual("fz_balance", NonlinearTerm(f0[2] - f1[2], gain=PAIR_GAINS[1]), nodes=range(0, ns))
    else:
        prb.createResidual("vx", LinearTerm({v["rdot"]: [[1, 0, 0]], v["r"]: [[0.2, 0, 0]]}, gain=PAIR_GAINS[0], ref=ref),
                           nodes=range(1, ns + 1))
        prb.createResidual("fz_balance", LinearTerm({v["f0"]: [[0, 0, 1]], v["f1"]: [[0, 0, -1]]}, gain=PAIR_GAINS[1]),
                           nodes=range(0, ns))
    return pb, prb


def srbd37_reach(ns, with_stage=True):
    """The example's srbd37 problem (leg-reach state term) plus, with_stage, a stage term on the forces tanh((f0_z - f2_z) / 100)."""
    pb, prb = example_module().build_problem(ns)
    if with_stage:
        import sympy
        f0, f2 = pb.f[0].sym(), pb.f[2].sym()
        prb.createResidual("f_balance", NonlinearTerm(sympy.tanh((f0[2] - f2[2]) / 100), gain=1e1), nodes=range(0, ns))
    return pb, prb


def spec_of(prb):
    nx = sum(v.getDim() for v in prb.getState().getVars())
    nu = sum(v.getDim() for v in prb.getInput().getVars())
    return userterms.spec_from_problem(prb, nx, nu)


NPB = 19      # parameter columns of the SRBD models in front of the 8 user columns


def user_case(case, N):
    pb, prb = {"srbd13_terrain": lambda: srbd13_terrain(N), "srbd37_reach": lambda: srbd37_reach(N),
               "srbd13_pair": lambda: srbd13_pair(N, True)}[case]()
    spec = spec_of(prb)
    return spec, userterms.register(spec)


def widen(params, spec, vary=0.0):
    """the batch's parameters plus the 8 user columns, filled from the parameters the spec's rows read (vary: a per-node ripple)"""
    B, K, _ = params.shape
    P = np.concatenate([params, np.zeros((B, K, 8))], axis=2)
    for j, (par, r) in enumerate(spec.cols):
        P[:, :, NPB + j] = par.values[r, :K][None] * (1.0 + vary * np.sin(np.arange(K) / 3.0))[None]
    return P


# horizon lengths the tests use (the generated code does not depend on N, but the node ranges are part of the declaration)
def all_specs():
    out = []
    for ns in (20, 30):
        out.append(spec_of(srbd13_terrain(ns)[1]))
        out.append(spec_of(srbd13_pair(ns, True)[1]))
    out.append(spec_of(srbd37_reach(20)[1]))
    out.append(spec_of(srbd37_reach(20, with_stage=False)[1]))
    return out


def prebuild(verbose=False):
    """Compile every user build the tests and the example use (in parallel; existing builds are kept)."""
    from concurrent.futures import ThreadPoolExecutor
    specs = {userterms.build_path(s): s for s in all_specs()}
    from srbd_horizon_amd import _lib
    workers = max(1, min(len(specs), _lib.build_jobs()))
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(lambda s: userterms.ensure_build(s, verbose), specs.values()))
