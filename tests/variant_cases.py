"""The problem variants several test modules solve -- the four linear user rows of the "_x" builds, the bound-barrier settings, a drawn
table of per-instance constants -- each stated once (no GPU needed: tests/sweep_cases.py builds its CPU references from them)."""
import dataclasses

import numpy as np

from oracle import cport, models as omodels
from srbd_horizon_amd import workload


def extra_rows(model):
    nx, nu, _ = cport.DIMS[model]
    nz = nx + nu
    rng = np.random.default_rng(5)
    a0 = np.zeros(nz); a0[0] = 1.0                                  # r_x tracking (state row)
    a1 = np.zeros(nz); a1[1] = 1.0; a1[0] = -0.5                    # r_y - r_x / 2 (state row)
    a2 = np.zeros(nz); a2[nx + 2] = 1.0; a2[nx + (5 if model != "lip30" else 1)] = -1.0       # a difference of inputs (stage row)
    a3 = np.zeros(nz); a3[:nx] = 0.05 * rng.standard_normal(nx); a3[nx:] = 0.05 * rng.standard_normal(nu)   # dense (stage row)
    return (dict(a=a0, w=2e3, kind="state", const=0.0), dict(a=a1, w=5e2, kind="state", const=0.01),
            dict(a=a2, w=3.0, kind="stage", const=0.0), dict(a=a3, w=40.0, kind="stage", const=-0.2))


def extra_rows_problem(model, N, seeds):
    batch = workload.make_batch(model, N, seeds)
    rows = extra_rows(model)
    npb = cport.DIMS[model][2]
    B = len(seeds)
    P = np.concatenate([batch["params"], np.zeros((B, N + 1, 8))], axis=2)
    P[:, :, npb + 0] = 0.02 * np.sin(np.arange(N + 1) / 5.0)[None]              # per-knot reference of row 0
    P[:, :, npb + 3] = 0.1 * np.cos(np.arange(N + 1) / 3.0)[None]               # ... and of row 3
    consts = dict(batch["consts"], extra_rows=rows)
    return batch, P, consts


def bounds(name):
    """CoM height band and a cap / floor on every vertical contact force (scaled forces: static load = 0.196 resp. 0.098)"""
    nx, nu = (13, 6) if name == "srbd13" else (37, 24)
    lo, up = np.full(nx + nu, -np.inf), np.full(nx + nu, np.inf)
    lo[2], up[2] = 0.80, 0.95
    fz = [nx + 2, nx + 5] if name == "srbd13" else [nx + 6 * i + 5 for i in range(4)]
    for j in fz:
        lo[j], up[j] = 0.0, (0.25 if name == "srbd13" else 0.125)
    return dict(bound_barrier_weight=1.0, bound_barrier_sharpness=6.0, lower=lo, upper=up)      # weight 1, exp_parameter 6: ddp.py:182, :205-208


def draw(consts: dict, B: int, fields, seed=2026):
    """Per instance, in this order: m x U(0.75, 1.25), I x U(0.8, 1.25), then every gain of `fields` x U(0.5, 2), from ONE
    default_rng(seed).  -> (overrides for set_instance_consts, [RobotConsts] for the oracle)"""
    base = omodels.RobotConsts(**consts)
    rng = np.random.default_rng(seed)
    over = {k: [] for k in ("m", "I", *fields)}
    csts = []
    for _ in range(B):
        v = dict(m=base.m * rng.uniform(0.75, 1.25), I=np.asarray(base.I, dtype=float) * rng.uniform(0.8, 1.25))
        for k in fields:
            v[k] = getattr(base, k) * rng.uniform(0.5, 2.0)
        for k in over:
            over[k].append(v[k])
        csts.append(dataclasses.replace(base, **v))
    return {k: np.asarray(v) for k, v in over.items()}, csts


SRBD13_FIELDS = ("r_tracking_gain", "rdot_tracking_gain", "w_tracking_gain", "min_f_gain")
TRACKING = ("r_tracking_gain", "rdot_tracking_gain", "w_tracking_gain")
