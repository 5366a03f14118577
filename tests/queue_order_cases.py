"""The queue orders (sddp_options.queue_order 1, 2, 3): the rules stated once in numpy, and the case table that
tests/test_queue_order_cases_cpu.py (can the table tell a right order from a wrong one? -- the oracles, no GPU) and
tests/test_gpu_queue_order.py (the order every kernel family hands its instances out in, read back through
DdpEngine.last_queue_order) share.

The order changes no byte of any result, so no parity test sees it; here it is the thing compared.  The rules:
  order 2   descending total cost J0 of the warm start (x_0 := x0); a non-finite J0 counts as +inf       order2_reference
  order 3   descending  mean + 1e-3 j0 / (|j0| + 1e9),  mean = the class's iterations / solves so far, 1e6 for label -1 and
            for a class without history; a non-finite j0 stays the key                                    order3_keys
  order 1   descending  min(iterations of the previous solve, 256),  257 for "never solved"               order1_keys
J0 comes from the C oracle (cport.solve_batch at max_iters = 0, the stats' "cost") with the case's model, constants and parameter rows,
instance by instance where the instances have constants of their own.  The one exception is the user build: its rows are
non-linear, which the C oracle does not have, so its J0 is oracle.ddp.total_cost of the numpy oracle wrapped with the same rows
(tests/user_terms_oracle.py); test_queue_order_cases_cpu.py asserts that this sum and the C oracle agree to 1e-12 on the same batch
without the rows.  Class sums and previous iteration counts are the rules' own inputs and are read from the handle.

Tolerance.  KEY_RTOL = 1e-9 relative to max |J0| (finite ones) is what the existing order-2 test allows: the GPU sums the knots in
another order than the oracle.  It is a cap that could hide a wrong order, so every case is chosen such that the reference alone has
no two finite keys closer than SEPARATION = 1e3 KEY_RTOL max |J0| (asserted on the CPU): "follows within the tolerance" then means
"equals the reference argsort", which the GPU test asserts outright.  Integer keys (order 1) have tolerance 0 and declared ties.
Order 3: the key is a double near the class mean, so the tie-break is only as fine as one ulp of that mean.  In units of J0 one ulp
is ulp(mean) (|j0| + 1e9)^2 / 1e6: 3.6e-3 at a mean of 16 .. 31, 1.8e-3 at 8 .. 15, and 116 at the 1e6 of an unlabelled instance or a
class without history (J0 of the srbd13 workload is 9e7: |j0| + 1e9 is 1.09e9, the figures are for j0 << 1e9 and 19 % larger there).  The reference keys are computed in float64 exactly as
documented; the tolerance is one ulp of the largest finite key, and a pair of reference keys inside it -- equal or adjacent
doubles -- is a declared tie (order3_ties counts them).  Such ties exist only in the 1e6 groups of the tables below and where the
table says so.

Key cases (queue_order 2, max_iters = 0: nothing iterates, stats.cost is J0).  B = 48 on max_slots = 4 unless stated.
  plain     srbd13 N = 30 (waves_per_simd 1 and 2), srbd37 N = 20, lip30 N = 20, srbd61 N = 12
  horizon   srbd13 N = 63, 64, 65, 129; srbd37 N = 65; lip30 N = 64 (B = 16): the second and third trip of the key kernel's
            one-lane-per-knot loop.  (At N = 63 the 64 knots are one trip: the "knots 0 .. 63 only" mutation is the truth there.)
  builds    srbd13 and srbd37 `_x` with the first three user rows of variant_cases.extra_rows (two state rows, one stage row) and
            the parameter columns of variant_cases.extra_rows_problem; srbd13 with the friction barrier, with the bound barrier
            (variant_cases.bounds), on the second_order = 2 build, and the srbd13_terrain user build of tests/user_terms_defs.py
            (pre-built by build(); registering it takes a dlopen, the test stays well under a second)
  table     srbd13 and srbd37 with per-instance constants (variant_cases.draw: mass, inertia and gains spread per instance)
  range     srbd13, handle of B = 64, one launch over first = 5, count = 50; the 14 instances outside hold other warm starts
  nonfinite srbd13, instance 7 = failure_cases S3a (a NaN in x0 and xs), instance 30 = S3d (x0[0] = 1e160: J0 overflows); both lead
            the queue under orders 2 and 3, in either order (one declared tie)

The warm starts.  workload.make_batch repeats x0 along the horizon and gives every instance the same static input: every knot then
carries the same state cost, J0 is the same sum with or without its last knot (or its second trip of 64 knots) up to a factor, and
the rows and barriers of the builds add the same constant to every instance -- no choice of seeds or constants lets such a batch tell
a key kernel that forgets a knot, a row or a barrier from a right one (measured: "no terminal cost" moves 0 to 2 of 48 positions).
The key cases therefore add seeded noise to the workload's warm start (_noisy_batch): NOISE_V = 3 x N(0, 1) on the CoM velocity of
the knots 1 .. N, which enters the state cost and the terminal cost and nothing else; on the `_x`, bound-barrier and user builds also
NOISE_R = 0.3 x N(0, 1) on the CoM position, which their rows and bounds read; on the friction-barrier build NOISE_U = 0.05 x N(0, 1)
on the inputs.  Constants replaced so that the rows and barriers weigh in the order: the user rows' weights x ROW_SCALE = 1e3, the
terrain term's gain 1e6 (runtime data of the same user build), bound_barrier_weight 1e4, friction_barrier_weight 1e5 (sharpness 4).
Seeds replaced for separation: srbd37-x (4850 for 4800: 5.2e-7), srbd13-range (5550 for 5500: 1.1e-6).  x0, the parameters and the
order 1 / order 3 cases are the workload's, untouched.

Measured on the C oracle (builds `off` and `fast` give the same argsort on every case; the figures are in MEASURED and asserted by
the CPU test): the smallest distance between two finite keys, relative to max |J0| (SEPARATION is 1e-6), and the share of queue
positions each mutation of the key moves (MUTATION_SHARE = 1/4 is asked of every one).
  srbd13-N30-w1      sep 3.4e-05   no terminal cost 0.77
  srbd13-N30-w2      sep 3.4e-05   no terminal cost 0.77
  srbd37-N20         sep 3.8e-06   no terminal cost 0.83
  lip30-N20          sep 8.9e-04   no terminal cost 0.81
  srbd61-N12         sep 1.6e-04   no terminal cost 0.71
  srbd13-N63         sep 7.8e-06   no terminal cost 0.58   (knots 0 .. 63 only: the truth, one trip)
  srbd13-N64         sep 2.2e-06   no terminal cost 0.56   knots 0 .. 63 only 0.56
  srbd13-N65         sep 2.9e-05   no terminal cost 0.44   knots 0 .. 63 only 0.81
  srbd13-N129        sep 9.4e-06   no terminal cost 0.27   knots 0 .. 63 only 0.96
  srbd37-N65         sep 3.7e-05   no terminal cost 0.60   knots 0 .. 63 only 0.79
  lip30-N64          sep 3.1e-03   no terminal cost 0.44   knots 0 .. 63 only 0.44
  srbd13-x           sep 7.6e-05   no terminal cost 0.62   without the user rows 0.98
  srbd37-x           sep 7.0e-05   no terminal cost 0.75   without the user rows 0.94
  srbd13-friction    sep 1.2e-05   no terminal cost 0.33   without the barrier 0.31
  srbd13-bound       sep 1.5e-05   no terminal cost 0.62   without the barrier 0.94
  srbd13-so2         sep 3.4e-05   no terminal cost 0.77   (the cost does not depend on second_order)
  srbd13-user        sep 1.2e-05   no terminal cost 0.85   without the user rows 0.88
  srbd13-table       sep 4.2e-05   no terminal cost 0.56   the handle's constants for every instance 1.00
  srbd37-table       sep 8.8e-05   no terminal cost 0.60   the handle's constants for every instance 0.96
  srbd13-range       sep 8.0e-06   no terminal cost 0.70   key[i] where the key of first + i belongs 0.94
  srbd13-nonfinite   sep 1.2e-05   no terminal cost 0.71
  every case: ascending instead of descending moves every position (the two non-finite leaders stay: 0.96)

Order 1:
  (a) srbd13 N = 30, B = 96, max_slots = 8: two launches; the second follows order1_keys(iterations of the first), exactly
  (b) the range [0, 48) solved first, then the whole batch: every instance of 48 .. 95 (never solved) before any of 0 .. 47
  (c) the clamp and the stride loop.  lip30 N = 5 is linear-quadratic: with alpha_0 = C_ALPHA0 = 0.05 the gaps shrink by 5 % per
      iteration and the C oracle (both builds) takes C_ITERS_FREE = 345 .. 373 iterations from the workload's 48 starts (seeds
      5000 ..) with max_iters = 500 (876 .. 947 at alpha_0 = 0.02, 1760 .. 1903 at 0.01), so a cap of 300, 257, 256 or 200 is the iteration count of every instance.  Four ranges of
      12 are solved at these caps, then the whole batch is queued: keys 256, 256, 256, 200.  The same shape on srbd13 N = 4 with
      B = 1500 (ranges of 375 at max_iters 100, 2, 1, the fourth never solved): count > 1024, the second trip of the kernel's loops.

Order 3 (labels: workload.srbd13_schedule_classes / workload.schedule_classes; one learning solve under BASE, then the launch that
is looked at, at max_iters = 0):
  (d) srbd13 N = 30, B = 192, max_slots = 16, waves_per_simd = 2; srbd37 N = 20, B = 24, max_slots = 2
  (e) every fifth instance unlabelled (-1) and the largest class labelled only after the learning solve: both lead, at 1e6
  (f) no class table on the handle: order 2's reference; run on the key cases srbd13-N30-w1 and srbd37-N20, whose keys are separated
      (the order 3 shapes are the workload's own starts: 192 of them lie as close as 3.7e-9 of max |J0|)
Inside a class the initial costs of the order 3 shapes are at least 39.7 (srbd13) and 2382 (srbd37) apart, four orders above the
tie-break's resolution at a mean below 32; with a history the reference keys of (d) have no tie.  In (e) 45 (srbd13) and 8 (srbd37)
instances lead at 1e6, where the resolution is 116: 3 and 0 declared ties.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import cport, ddp as oddp, models as omodels
from srbd_horizon_amd import workload
from tests import failure_cases as fc, oracle_refs as refs, user_terms_defs as defs, variant_cases
from tests.user_terms_oracle import WithUserRows

BASE = refs.BASE
KEY_RTOL = 1e-9
SEPARATION = 1e-6                     # relative to max |J0|: no two finite reference keys of a case are closer
MUTATION_SHARE = 0.25                  # of the queue positions: what every mutation of a case's key must move
B, SLOTS = 48, 4

FRICTION = dict(friction_barrier_weight=1e5, friction_barrier_sharpness=4.0)
USER_CASE, USER_VARY, USER_GAIN = "srbd13_terrain", 0.1, 1e6
ROW_SCALE, BOUND_WEIGHT = 1e3, 1e4
NAN_AT, INF_AT = 7, 30                 # the non-finite case: where the S3a and the S3d instance sit

Case = namedtuple("Case", "name kind model N B seeds build wps slots first count")


def _key(name, kind, model, N, seed0, build="plain", wps=0, batch=B, slots=SLOTS, first=0, count=None):
    return Case(name, kind, model, N, batch, tuple(range(seed0, seed0 + batch)), build, wps, slots, first, batch if count is None else count)


def key_cases():
    out = [_key("srbd13-N30-w1", "plain", "srbd13", 30, 4000, wps=1), _key("srbd13-N30-w2", "plain", "srbd13", 30, 4000, wps=2),
           _key("srbd37-N20", "plain", "srbd37", 20, 4100), _key("lip30-N20", "plain", "lip30", 20, 4200),
           _key("srbd61-N12", "plain", "srbd61", 12, 4300)]
    out += [_key(f"srbd13-N{N}", "horizon", "srbd13", N, 4400) for N in (63, 64, 65, 129)]
    out += [_key("srbd37-N65", "horizon", "srbd37", 65, 4500), _key("lip30-N64", "horizon", "lip30", 64, 4600, batch=16)]
    out += [_key("srbd13-x", "builds", "srbd13", 30, 4700, "x"), _key("srbd37-x", "builds", "srbd37", 20, 4850, "x"),
            _key("srbd13-friction", "builds", "srbd13", 30, 4900, "friction"), _key("srbd13-bound", "builds", "srbd13", 30, 5100, "bound"),
            _key("srbd13-so2", "builds", "srbd13", 30, 4000, "so2"), _key("srbd13-user", "builds", "srbd13", 30, 5200, "user")]
    out += [_key("srbd13-table", "table", "srbd13", 30, 5300, "table"), _key("srbd37-table", "table", "srbd37", 20, 5400, "table")]
    out.append(_key("srbd13-range", "range", "srbd13", 30, 5550, batch=64, first=5, count=50))
    out.append(_key("srbd13-nonfinite", "nonfinite", "srbd13", 30, 5600))
    return out


KEY_CASES = {c.name: c for c in key_cases()}

# smallest relative distance of two finite keys, and the share of positions each mutation moves: measured (module docstring); the CPU
# test asserts SEPARATION and MUTATION_SHARE, and that the measured figures have not drifted below half of what is written here
MEASURED = {
    "srbd13-N30-w1": dict(sep=3.36e-05, no_terminal=0.771), "srbd13-N30-w2": dict(sep=3.36e-05, no_terminal=0.771),
    "srbd37-N20": dict(sep=3.83e-06, no_terminal=0.833), "lip30-N20": dict(sep=8.92e-04, no_terminal=0.812),
    "srbd61-N12": dict(sep=1.64e-04, no_terminal=0.708),
    "srbd13-N63": dict(sep=7.75e-06, no_terminal=0.583), "srbd13-N64": dict(sep=2.21e-06, no_terminal=0.562, one_trip=0.562),
    "srbd13-N65": dict(sep=2.89e-05, no_terminal=0.438, one_trip=0.812), "srbd13-N129": dict(sep=9.36e-06, no_terminal=0.271, one_trip=0.958),
    "srbd37-N65": dict(sep=3.67e-05, no_terminal=0.604, one_trip=0.792), "lip30-N64": dict(sep=3.08e-03, no_terminal=0.438, one_trip=0.438),
    "srbd13-x": dict(sep=7.59e-05, no_terminal=0.625, plain_build=0.979), "srbd37-x": dict(sep=7.02e-05, no_terminal=0.750, plain_build=0.938),
    "srbd13-friction": dict(sep=1.18e-05, no_terminal=0.333, plain_build=0.312),
    "srbd13-bound": dict(sep=1.55e-05, no_terminal=0.625, plain_build=0.938),
    "srbd13-so2": dict(sep=3.36e-05, no_terminal=0.771), "srbd13-user": dict(sep=1.19e-05, no_terminal=0.854, plain_build=0.875),
    "srbd13-table": dict(sep=4.18e-05, no_terminal=0.562, handle_consts=1.000),
    "srbd37-table": dict(sep=8.82e-05, no_terminal=0.604, handle_consts=0.958),
    "srbd13-range": dict(sep=8.04e-06, no_terminal=0.700, range_swapped=0.940), "srbd13-nonfinite": dict(sep=1.19e-05, no_terminal=0.708),
}

# order 1, case (c): measured on the C oracle, both builds
C_MODEL, C_N, C_SEED0, C_ALPHA0 = "lip30", 5, 5000, 0.05
C_CAPS = (300, 257, 256, 200)
C_RANGE = B // len(C_CAPS)
C_FREE_MAX_ITERS, C_ITERS_FREE = 500, (345, 373)      # the oracle's iteration counts without a binding cap: smallest, largest
STRIDE = dict(model="srbd13", N=4, B=1500, seed0=6000, slots=64, caps=(100, 2, 1))      # the fourth range of 375 is never solved

# order 3: model -> (N, B, max_slots, waves_per_simd, first seed)
ORDER3 = {"srbd13": (30, 192, 16, 2, 100), "srbd37": (20, 24, 2, 1, 7000)}
UNLABELLED_EVERY = 5


# ---- the rules ---------------------------------------------------------------------------------------------------------------------
def order2_reference(J0):
    """the key of queue order 2: J0, a non-finite one as +inf"""
    k = np.array(J0, dtype=np.float64)
    k[~np.isfinite(k)] = np.inf
    return k


def order3_keys(J0, labels, class_sum, class_count):
    """the key of queue order 3 as include/sddp.h documents it, in float64: the class mean (1e6 for label -1, a label outside the
    table and a class without history) + 1e-3 j0 / (|j0| + 1e9); a non-finite j0 stays the key (+inf: order2_reference)"""
    j0 = order2_reference(J0)
    labels = np.asarray(labels, dtype=np.int64)
    s, n = np.asarray(class_sum, dtype=np.float64), np.asarray(class_count, dtype=np.float64)
    mean = np.full(j0.shape, 1e6)
    c = np.clip(labels, 0, len(n) - 1)
    known = (labels >= 0) & (labels < len(n)) & (n[c] > 0)
    mean[known] = s[c[known]] / n[c[known]]
    fin = np.isfinite(j0)
    key = j0.copy()
    key[fin] = mean[fin] + 1e-3 * j0[fin] / (np.abs(j0[fin]) + 1e9)
    return key


def order1_keys(prev_iters):
    """the key of queue order 1: 257 for an instance never solved (-1), else min(iterations of its previous solve, 256)"""
    it = np.asarray(prev_iters, dtype=np.int64)
    return np.where(it < 0, 257, np.minimum(it, 256))


def _steps(k):
    """k[i + 1] - k[i]; 0 between two equal keys (two +inf as well)"""
    with np.errstate(invalid="ignore"):
        return np.where(k[1:] == k[:-1], 0.0, k[1:] - k[:-1])


def assert_follows(order, keys, first, count, tol):
    """`order`: what the launch over the instances [first, first + count) handed out; `keys`: the reference key of every instance
    of the handle, by absolute index.  order[:count] is a permutation of first .. first + count - 1 and keys[order] never rises by
    more than tol.  -> the number of adjacent pairs inside tol (ties the tolerance could hide: the caller asserts how many it
    declares)."""
    order = np.asarray(order)[:count].astype(np.int64)
    assert order.shape == (count,), f"the order has {order.shape[0]} entries, the launch {count}"
    assert order.min() >= first and order.max() < first + count, f"an index outside [{first}, {first + count}): {order.min()} .. {order.max()}"
    missing = np.setdiff1d(np.arange(first, first + count), order)
    assert missing.size == 0, f"not a permutation: {missing.tolist()[:8]} missing"
    d = _steps(np.asarray(keys, dtype=np.float64)[order])
    up = np.flatnonzero(d > tol)
    assert up.size == 0, (f"the key rises along the queue at positions {up.tolist()[:8]} (instances {order[up].tolist()[:8]} before "
                          f"{order[up + 1].tolist()[:8]}), by up to {d.max():.3e} > tol {tol:.3e}")
    return int((np.abs(d) <= tol).sum())


def reference_order(keys, first, count):
    """the instances of [first, first + count) by descending key (ties by index)"""
    return first + np.argsort(-np.asarray(keys, dtype=np.float64)[first:first + count], kind="stable")


def key_tol(J0):
    """KEY_RTOL max |J0| over the finite ones"""
    J0 = np.asarray(J0)
    return KEY_RTOL * np.abs(J0[np.isfinite(J0)]).max()


def separation(keys):
    """the smallest distance between two finite keys, relative to the largest finite |key|"""
    k = np.sort(np.asarray(keys)[np.isfinite(keys)])
    return np.diff(k).min() / np.abs(k).max()


def moved_share(keys, mutant, first, count):
    """the share of queue positions at which the order by `mutant` hands out another instance than the order by `keys`"""
    return float((reference_order(keys, first, count) != reference_order(mutant, first, count)).mean())


def order3_tol(keys):
    """one ulp of the largest finite key: equal or adjacent doubles are a tie"""
    k = np.asarray(keys)
    return float(np.spacing(np.abs(k[np.isfinite(k)]).max()))


def order3_ties(keys, first, count):
    """adjacent pairs of the sorted reference keys inside order3_tol: the declared ties"""
    k = np.asarray(keys, dtype=np.float64)[first:first + count]
    return int((np.abs(_steps(-np.sort(-k))) <= order3_tol(k)).sum())


def order1_ties(keys):
    """integer keys: any order that follows them has len - (distinct keys) adjacent equal pairs"""
    return len(keys) - len(np.unique(keys))


# ---- the key cases: inputs and references -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def user_spec(N):
    return defs.spec_of(defs.srbd13_terrain(N, gain=USER_GAIN)[1])


NOISE_V, NOISE_R, NOISE_U, NOISE_SEED = 3.0, 0.3, 0.05, 20260


def _noisy_batch(model, N, seeds, inputs=False, position=False):
    """workload.make_batch with seeded noise on the warm start: NOISE_V N(0, 1) on the CoM velocity of the knots 1 .. N and, with
    `inputs`, NOISE_U N(0, 1) on every input (module docstring)"""
    b = refs.batch(model, N, seeds)
    rng = np.random.default_rng(NOISE_SEED + int(seeds[0]))
    xs, us = b["xs"].copy(), b["us"].copy()
    rd = omodels.make_model(model).RD_
    xs[:, 1:, rd] += NOISE_V * rng.standard_normal(xs[:, 1:, rd].shape)
    if position:
        xs[:, 1:, 0:3] += NOISE_R * rng.standard_normal(xs[:, 1:, 0:3].shape)
    if inputs:
        us += NOISE_U * rng.standard_normal(us.shape)
    return dict(b, xs=xs, us=us)


@functools.lru_cache(maxsize=None)
def start(name):
    """-> dict(x0, params, xs, us: the whole handle's, read-only; consts: the engine's constants; plain: the constants and parameters
    of the plain build on the same batch (None where the case is one); table: the per-instance overrides or None; csts: one
    RobotConsts per instance; opts: what the case adds to the options)"""
    c = KEY_CASES[name]
    b = _noisy_batch(c.model, c.N, c.seeds, inputs=c.build == "friction", position=c.build in ("x", "bound", "user"))
    out = {k: b[k].copy() for k in ("x0", "params", "xs", "us")}
    consts, plain, table, opts = dict(b["consts"]), None, None, {}
    if c.build != "plain":
        plain = (dict(b["consts"]), b["params"])
    if c.build == "x":
        out["params"] = variant_cases.extra_rows_problem(c.model, c.N, list(c.seeds))[1]
        consts["extra_rows"] = tuple(dict(r, w=ROW_SCALE * r["w"]) for r in variant_cases.extra_rows(c.model)[:3])
    elif c.build == "friction":
        consts.update(FRICTION)
    elif c.build == "bound":
        consts.update(variant_cases.bounds(c.model), bound_barrier_weight=BOUND_WEIGHT)
    elif c.build == "so2":
        opts, plain = dict(second_order=2), None
    elif c.build == "user":
        spec = user_spec(c.N)
        out["params"] = defs.widen(b["params"], spec, vary=USER_VARY)
        consts["extra_rows"] = spec.extra_rows()
    csts = [omodels.RobotConsts(**(b["consts"] if c.build == "user" else consts))] * c.B
    if c.build == "table":
        table, csts = variant_cases.draw(consts, c.B, variant_cases.SRBD13_FIELDS if c.model == "srbd13" else variant_cases.TRACKING)
    if c.kind == "nonfinite":                             # the failing instance 0 of failure_cases S3a and S3d (same model and horizon)
        for at, kind in ((NAN_AT, "S3a"), (INF_AT, "S3d")):
            f = fc.start(f"{kind}-{c.model}")
            assert fc.CASES[f"{kind}-{c.model}"].N == c.N and 0 in fc.CASES[f"{kind}-{c.model}"].fail
            for k in ("x0", "xs", "us", "params"):
                out[k][at] = f[k][0]
    out = refs.frozen(out)
    out.update(consts=consts, plain=plain, table=table, csts=csts, opts=opts)
    return out


def _c_costs(model, csts, s, P, variant):
    """J0 of every instance from the C oracle: one call where the instances share their constants, else instance by instance"""
    def cost(c, sel):
        return cport.stat(refs.c_oracle(model, s, refs.options({}, max_iters=0), variant, cst=c, sel=sel, params=P)[2], "cost")
    if all(c is csts[0] for c in csts):
        return cost(csts[0], slice(None)).copy()
    return np.array([cost(c, [b])[0] for b, c in enumerate(csts)])


def _user_model(name):
    c, s = KEY_CASES[name], start(name)
    return WithUserRows(omodels.make_model(c.model, s["csts"][0]), user_spec(c.N))


@functools.lru_cache(maxsize=None)
def initial_costs(name, variant="off"):
    """-> J0 [B] of every instance of the case's handle (module docstring), read-only"""
    c, s = KEY_CASES[name], start(name)
    if c.build == "user":
        m = _user_model(name)
        xs = s["xs"].copy(); xs[:, 0] = s["x0"]
        J = np.array([oddp.total_cost(m, xs[b], s["us"][b], s["params"][b]) for b in range(c.B)])
    else:
        J = _c_costs(c.model, s["csts"], s, s["params"], variant)
    return refs.frozen(J)


def _knot_cost(name, b, k):
    """the cost of knot k of instance b of the case (x_0 = x0)"""
    c, s = KEY_CASES[name], start(name)
    x = s["x0"][b] if k == 0 else s["xs"][b, k]
    if c.build == "user":
        return _user_model(name).cost(x, None if k == c.N else s["us"][b, k], s["params"][b, k], k)
    u = np.zeros(cport.DIMS[c.model][1]) if k == c.N else s["us"][b, k]
    return cport.eval_knot(s["csts"][b], x, u, s["params"][b, k], k, k == c.N, model=c.model)[4]


ONE_TRIP = 64                                             # lanes of the key kernel: the knots 0 .. 63 are its first trip


@functools.lru_cache(maxsize=None)
def mutants(name):
    """-> {mutation: keys [B]} of what a wrong key kernel or a wrong sort would order the case by:
      no_terminal    J0 without the cost of knot N
      one_trip       J0 over the knots 0 .. min(N, 63) only (horizon cases with N >= 64)
      handle_consts  every instance priced with the handle's constants (table cases)
      plain_build    J0 without the user rows / the barrier (those builds)
      range_swapped  the key of instance i where first + i belongs (the range case)
      ascending      the sort direction"""
    c, s = KEY_CASES[name], start(name)
    J = order2_reference(initial_costs(name))
    live = [b for b in range(c.B) if np.isfinite(J[b])]
    out = {"ascending": np.where(np.isfinite(J), -J, J)}
    tail = {b: [_knot_cost(name, b, k) for k in range(min(c.N, ONE_TRIP), c.N + 1)] for b in live}      # knots 64 .. N (N >= 64), N
    for mut, n in (("no_terminal", 1), ("one_trip", c.N + 1 - ONE_TRIP)):
        if n >= 1 and (mut == "no_terminal" or c.kind == "horizon"):
            m = J.copy()
            for b in live:
                m[b] = J[b] - sum(tail[b][-n:])
            out[mut] = m
    if c.build == "table":
        out["handle_consts"] = _c_costs(c.model, [omodels.RobotConsts(**s["consts"])] * c.B, s, s["params"], "off")
    if s["plain"] is not None and c.build != "table":
        out["plain_build"] = _c_costs(c.model, [omodels.RobotConsts(**s["plain"][0])] * c.B, s, s["plain"][1], "off")
    if c.first:
        m = J.copy()
        m[c.first:c.first + c.count] = J[:c.count]
        out["range_swapped"] = m
    return out


# ---- order 1, case (c), and the order 3 shapes -------------------------------------------------------------------------------------
def c_options(**more):
    return refs.options(dict(alpha_0=C_ALPHA0), **more)


@functools.lru_cache(maxsize=None)
def c_start():
    return refs.batch(C_MODEL, C_N, range(C_SEED0, C_SEED0 + B))


@functools.lru_cache(maxsize=None)
def c_oracle_iters(max_iters, variant="off", first=0, count=B):
    """-> the C oracle's iteration counts [count] of case (c) at that cap"""
    st = refs.c_oracle(C_MODEL, c_start(), c_options(max_iters=max_iters), variant, sel=slice(first, first + count))[2]
    return cport.stat(st, "iters").astype(int)


@functools.lru_cache(maxsize=None)
def stride_start():
    return refs.batch(STRIDE["model"], STRIDE["N"], range(STRIDE["seed0"], STRIDE["seed0"] + STRIDE["B"]))


@functools.lru_cache(maxsize=None)
def order3_start(model):
    """-> dict(x0, params, xs, us, consts, labels, n_classes, J0) of the order 3 shape of `model`, read-only"""
    N, B3, _, _, seed0 = ORDER3[model]
    out = refs.batch(model, N, range(seed0, seed0 + B3))
    out["labels"], out["n_classes"] = (workload.srbd13_schedule_classes if model == "srbd13" else functools.partial(workload.schedule_classes, model))(out["params"])
    out["J0"] = _c_costs(model, [refs.consts(out)] * B3, out, out["params"], "off")
    return out


def order3_labels_e(model):
    """case (e) -> (labels while the handle learns, labels of the launch looked at, the class without history): every fifth instance
    unlabelled in both; the largest class unlabelled while learning, labelled afterwards"""
    lab = order3_start(model)["labels"]
    final = lab.copy()
    final[::UNLABELLED_EVERY] = -1
    present, n = np.unique(final[final >= 0], return_counts=True)
    unseen = int(present[np.argmax(n)])
    learning = final.copy()
    learning[final == unseen] = -1
    return learning, final, unseen
