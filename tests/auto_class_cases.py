"""Hand-built inputs of the class labelling (include/sddp.h sddp_enable_auto_classes; workload.schedule_classes states the formula).

`build(model, N, B, extra)` takes a parameter tensor from workload.make_batch and overwrites the two switch columns and the two
command columns of every instance by hand, one designated case per instance (`cases(N)`, repeated when B is larger).  The label
each case must get is written down with the case -- stance0 and first_change as literals, the command classes from CMD_CLASS -- and
NOT computed by the function under test.  What the cases cover:

  * all four stance patterns at node 0;
  * first_change at 1, 2, N - 1, N and never (N + 1); for N + 1 > 64 (two chunks of the kernel's 64 nodes per step) at 63, 64, 65
    and in the last node;
  * a change in the right foot's column only, in the left one only, in both; a change that is undone later (the FIRST one counts);
  * a switch value of exactly 0.5 (not in stance) at node 0 and later; values that are neither 0 nor 1 (0.7 / 0.3 / 0.4);
  * a NaN in a switch column: at node 0 (not in stance), later against a foot in stance (a change) and against one that is not
    (no change);
  * the commands 0.0, -0.0, +-1e-12 (class 0), +-2e-12 and +-0.5, each in both command columns; the command is read at node N only:
    the earlier nodes hold a decoy of the opposite sign.

Everything is built once per (model, N, B, extra) and handed out read-only."""
import functools

import numpy as np

from srbd_horizon_amd import workload
from tests import oracle_refs as refs

NAN = float("nan")
CMDS = (0.0, -0.0, 1e-12, -1e-12, 2e-12, -2e-12, 0.5, -0.5)
CMD_CLASS = (0, 0, 0, 0, 1, 2, 1, 2)       # 0: |v| <= 1e-12, 1: v > 1e-12, 2: v < -1e-12
L, R = 0, 1


def cases(N):
    """-> list of (l0, r0, writes, stance0, first_change): the left / right switch column holds l0 / r0 at every node, then each
    write (k, foot, value) sets that foot's column from node k to the end, in order."""
    assert N >= 8
    c = [
        (1.0, 1.0, (), 3, N + 1),                                            # never
        (1.0, 0.0, ((1, L, 0.0),), 2, 1),                                    # left only, at the first node it can be
        (0.0, 1.0, ((2, R, 0.0),), 1, 2),                                    # right only
        (0.0, 0.0, ((N, L, 1.0), (N, R, 1.0)), 0, N),                        # both, in the last node
        (1.0, 1.0, ((3, L, 0.5),), 3, 3),                                    # exactly 0.5 is not in stance
        (0.5, 1.0, (), 1, N + 1),                                            # ... at node 0 too
        (1.0, 1.0, ((4, R, NAN),), 3, 4),                                    # NaN is not in stance: a change against 1
        (NAN, 1.0, ((2, L, 0.0),), 1, N + 1),                                # ... and none against 0; NaN at node 0
        (1.0, 0.0, ((1, R, 1.0), (2, R, 0.0), (5, L, 0.0)), 2, 1),           # undone at 2, another change at 5: the first counts
        (0.7, 0.3, ((N - 1, L, 0.4),), 2, N - 1),                            # neither 0 nor 1
        (1.0, 1.0, ((2, R, 0.0), (3, R, 1.0)), 3, 2),
        (0.0, 0.0, (), 0, N + 1),                                            # the smallest label
        (1.0, 1.0, ((N, R, 0.0),), 3, N),                                    # right only, in the last node: towards the largest label
    ]
    if N + 1 > 64:                                                           # the second chunk of 64 nodes
        c += [
            (1.0, 0.0, ((63, L, 0.0),), 2, 63),                              # the last node of the first chunk
            (0.0, 1.0, ((64, R, 0.0),), 1, 64),                              # the first node of the second, right only
            (1.0, 1.0, ((65, L, 0.0),), 3, 65),
            (1.0, 1.0, ((64, L, NAN), (66, L, 1.0)), 3, 64),
            (0.0, 1.0, ((N, L, 0.6),), 1, N),                                # the last node, in the second chunk
        ]
    return c


def command(b):
    """the indices into CMDS of instance b's two commands: both run through all eight values over eight consecutive instances"""
    return b % 8, (3 * b + 1) % 8


@functools.lru_cache(maxsize=None)
def build(model, N, B, extra=0):
    """-> dict(x0, xs, us, params [B, N+1, np + extra], consts, labels [B] int32, n_classes, stance0 [B], first_change [B]): a
    make_batch problem whose switch and command columns are the cases'.  extra: zero columns behind the model's own (the user rows'
    reference columns of an `_x` handle: extra = 8)."""
    batch = workload.make_batch(model, N, np.arange(B) + 300)
    cols = workload.CLASS_COLUMNS[model]
    P = np.concatenate([batch["params"], np.zeros((B, N + 1, extra))], axis=2)
    cs = cases(N)
    labels, stance, change = np.empty(B, np.int32), np.empty(B, np.int64), np.empty(B, np.int64)
    for b in range(B):
        l0, r0, writes, s0, fc = cs[b % len(cs)]
        P[b, :, cols["sw"][L]] = l0
        P[b, :, cols["sw"][R]] = r0
        for k, foot, v in writes:
            P[b, k:, cols["sw"][foot]] = v
        ix, iy = command(b)
        P[b, :N, cols["cmd"][0]] = -0.25 if CMDS[ix] >= 0 else 0.25           # decoys: the command is node N's
        P[b, :N, cols["cmd"][1]] = -0.25 if CMDS[iy] > 0 else 0.25
        P[b, N, cols["cmd"][0]] = CMDS[ix]
        P[b, N, cols["cmd"][1]] = CMDS[iy]
        labels[b] = ((s0 * (N + 2) + fc) * 3 + CMD_CLASS[ix]) * 3 + CMD_CLASS[iy]
        stance[b], change[b] = s0, fc
    out = dict(x0=batch["x0"], xs=batch["xs"], us=batch["us"], params=P, labels=labels, stance0=stance, first_change=change)
    refs.frozen(out.values())
    out.update(consts=batch["consts"], n_classes=36 * (N + 2))
    return out
