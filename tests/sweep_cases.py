"""One backward sweep and one rollout in the configurations a solve runs after its first full step: the case table that
tests/test_sweep_cases_cpu.py (is every case well-conditioned, and would a wrong term show? -- numpy oracle only) and
tests/test_gpu_sweep_modes.py (the kernels against the numpy oracle) share.

The phase-level entry points (sddp_backward / sddp_forward) ran one configuration only: Gauss-Newton sweep (theta = 0), open gaps,
mu = 0.  DdpEngine.backward(params, mu, theta, closed) / forward(params, alpha, closed) reach the others (sddp_debug_set_phase_mode):
the bilinear-torque term v'.f_ux of second_order = 1, the v'.f_zz tensor and exact wdot Hessian of the second_order = 2 builds, the
closed-gap path of the one-wave sweep and rollout (v' = Vx, no Vxx d product, no (1 - alpha) d correction) and mu > 0.

A case = model, kernel build, horizon, two workload seeds (B = 2), gaps, theta, mu.
  * The iterate is the numpy oracle's own solve (options BASE, second_order as the build) cut at max_iters = CUT.
  * The trajectory of a case is that iterate plus NOISE x N(0, 1) on every state and input, the recipe of
    test_backward_and_forward_pass_match_oracle (x_0 stays the initial state): its defects are ~1e-3, not rounding.
  * Where that start is no use -- the oracle itself rejects the theta = 1 sweep there (non-positive pivot), or its alpha = 1
    rollout overflows -- START names another one, found on the oracle alone: srbd13 at N = 65 and the second_order = 2 build at
    N = 30 take the seeds 1 and 6 (which converge; 2 and 9 crawl on long horizons) cut at 6 iterations, N = 65 with noise 3e-4;
    srbd37 at N = 20 takes noise 3e-4 (rejected at 1e-3 at every cut 2..10); srbd61 at N = 6 is cut at 3.
  * gaps "open": the reference sweeps with the trajectory's defects d.  gaps "closed": the reference takes d = 0 on the SAME
    trajectory -- the kernel is told that the gaps count as closed and must not read the defects; a kernel that did would miss by
    the margin test_sweep_cases_cpu.py asserts (condition b).
  * Reference: oracle.ddp.backward_pass(m, xs, us, P, d, mu, theta, mode), mode = 2 on a second_order = 2 build, else 1; the
    rollouts are oracle.ddp.forward_pass with THOSE gains at the step lengths ALPHAS.
  * Rejection cases: the iterate itself (no noise), theta = 1, mu = 1e-6, where the oracle's sweep meets a non-positive pivot
    (ok = False: what decides the theta -> 0 fallback of a solve).  Kept only where 8 copies of the iterate perturbed by 1e-10
    relative give the same verdict.  srbd13 plain N = 30 seeds 0 and 7 at CUT = 2; srbd37 second_order = 2, N = 20: a search
    over seeds 0..31 and cuts 1..4 found cut 1: every seed but 19; cut 2: seeds 2, 7, 11, 17, 22, 27; cuts 3 and 4: seed 12.
    Seeds 2 and 7 at cut 2 are the case.

Tolerances are the project's for one sweep (tests/test_gpu_parity.py, policy_cases.assert_policy_matches): gains rtol 1e-7, atol
1e-8 x max(1, max|ref|); dV1, dV2, G1, G2, qu_inf 1e-8 x max(1, |ref|, |dV1|); total cost 1e-11 relative; rollout x, u 1e-8, its
cost 1e-9 relative.  No case has a tolerance of its own.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import ddp as oddp, models as omodels
from tests import oracle_refs as refs, variant_cases

BASE = refs.BASE
CUT = 2
NOISE = 1e-3
ALPHAS = (1.0, 0.25, 2.0 ** -10)
SEEDS = {"srbd13": (2, 9), "srbd37": (3, 8), "srbd61": (1, 4), "lip30": (5, 0)}
FRICTION = dict(friction_barrier_weight=2.0, friction_barrier_sharpness=4.0)      # as test_full_second_order_mode_other_constants_...
PROBE_A, PROBE_REJECT = 1e-13, 1e-10      # relative perturbations of conditions (a) and of the rejection verdict

# (model, build, N) -> (cut, noise, seeds or None) where CUT, NOISE and SEEDS give no usable start (module docstring)
START = {("srbd13", "so2", 30): (6, 1e-3, (1, 6)), ("srbd13", "plain", 65): (6, 3e-4, (1, 6)),
         ("srbd37", "plain", 20): (CUT, 3e-4, None), ("srbd37", "so2", 20): (CUT, 3e-4, None), ("srbd61", "plain", 6): (3, 1e-3, None)}

# kernel builds: name -> (second_order = 2 build, constants on top of the workload's)
BUILDS = {"plain": (False, {}), "so2": (True, {}), "so2-conv": (True, dict(inertia_mode=1, lever_sign=-1.0)),
          "so2-friction": (True, FRICTION), "friction": (False, FRICTION), "bound": (False, "bounds"),
          "x": (False, "rows"), "table": (False, "table")}

Case = namedtuple("Case", "name model build N seeds cut noise gaps theta mu reject")


def _case(model, build, N, gaps, theta, mu, seeds=None, reject=False):
    name = f"{model}-{build}-N{N}-{gaps}-th{int(theta)}-mu{mu:g}" + ("-reject" if reject else "")
    cut, noise, seeds_ = START.get((model, build, N), (CUT, NOISE, None))
    return Case(name, model, build, N, tuple(seeds or seeds_ or SEEDS[model]), cut, 0.0 if reject else noise, gaps, float(theta), float(mu), reject)


def cases():
    out = []
    for N in (1, 3, 65):                                  # 65: one knot past a wavefront
        out += [_case("srbd13", "plain", N, g, th, mu) for g in ("open", "closed") for th in (0, 1) for mu in (0.0, 1e-6, 1e-2)]
    out += [_case("srbd13", "so2", N, g, 1, 1e-6) for N in (1, 3, 30) for g in ("open", "closed")]
    out += [_case("srbd13", b, 3, "closed", 1, 1e-6) for b in ("so2-conv", "so2-friction", "friction", "bound", "table")]
    out.append(_case("srbd13", "x", 3, "open", 1, 1e-6))
    out += [_case("srbd37", b, N, "open", th, mu) for b in ("plain", "so2") for N in (2, 20) for th in (0, 1) for mu in (0.0, 1e-6)]
    out.append(_case("srbd37", "so2-friction", 2, "open", 1, 1e-6))
    out += [_case("srbd61", "plain", N, "open", 1, 1e-6) for N in (1, 6)]
    out += [_case("lip30", "plain", N, "open", 1, 1e-6) for N in (2, 20)]
    out.append(_case("srbd13", "plain", 30, "open", 1, 1e-6, seeds=(0, 7), reject=True))
    out.append(_case("srbd37", "so2", 20, "open", 1, 1e-6, seeds=(2, 7), reject=True))
    return out


CASES = {c.name: c for c in cases()}
# one case per kernel family for tests/test_gpu_lds_poison.py
POISON_CASES = ("srbd13-plain-N3-closed-th1-mu1e-06", "srbd37-so2-N20-open-th1-mu1e-06")


def mode_of(case):
    return 2 if BUILDS[case.build][0] else 1


def options(case):
    """the handle's options; the oracle solve that makes the iterate runs with the same ones, cut at case.cut"""
    return dict(BASE, second_order=mode_of(case))


@functools.lru_cache(maxsize=None)
def _start(model, build, N, seeds, cut):
    """-> dict(x0, params, xs, us: the iterate, consts: the engine's constants, table: the per-instance overrides or None,
    models: one oracle model per instance); read-only"""
    so2, extra = BUILDS[build]
    B = len(seeds)
    batch = refs.batch(model, N, seeds)
    P, consts, table = batch["params"], dict(batch["consts"]), None
    if extra == "rows":                                   # the four user rows of tests/test_gpu_extra_rows.py
        _, P, consts = variant_cases.extra_rows_problem(model, N, list(seeds))
    elif extra == "bounds":
        consts.update(variant_cases.bounds(model))
    elif extra != "table":
        consts.update(extra)
    csts = [omodels.RobotConsts(**consts)] * B
    if extra == "table":                                  # two different robots in one handle (sddp_set_instance_consts)
        table, csts = variant_cases.draw(consts, B, variant_cases.SRBD13_FIELDS)
        assert csts[0].m != csts[1].m
    models = [omodels.make_model(model, c) for c in csts]
    opt = oddp.DdpOptions(**dict(BASE, second_order=2 if so2 else 1, max_iters=cut))
    res = [oddp.solve(models[b], batch["x0"][b], P[b], batch["xs"][b], batch["us"][b], opt) for b in range(B)]
    return refs.frozen(dict(x0=batch["x0"], params=np.ascontiguousarray(P), xs=np.stack([r.xs for r in res]), us=np.stack([r.us for r in res]),
                            consts=consts, table=table, models=models))


def start(case):
    return _start(case.model, case.build, case.N, case.seeds, case.cut)


@functools.lru_cache(maxsize=None)
def _trajectory(model, build, N, seeds, cut, noise):
    s = _start(model, build, N, seeds, cut)
    xs, us = s["xs"].copy(), s["us"].copy()
    if noise:
        rng = np.random.default_rng(1)
        xs += noise * rng.standard_normal(xs.shape)
        us += noise * rng.standard_normal(us.shape)
        xs[:, 0] = s["x0"]
    return refs.frozen((xs, us))


def trajectory(case):
    """-> xs [B, N+1, nx], us [B, N, nu] the case sweeps at, read-only"""
    return _trajectory(case.model, case.build, case.N, case.seeds, case.cut, case.noise)


Sweep = namedtuple("Sweep", "ok K kff dV1 dV2 G1 G2 qu_inf")


def sweep(case, b, xs=None, us=None, theta=None, mode=None, gaps=None):
    """the oracle's sweep of instance b; every argument defaults to the case's own"""
    s = start(case)
    if xs is None:
        xs, us = (a[b] for a in trajectory(case))
    m, P = s["models"][b], s["params"][b]
    gaps = case.gaps if gaps is None else gaps
    d = oddp.defects(m, xs, us, P) if gaps == "open" else np.zeros((case.N, m.nx))
    r = oddp.backward_pass(m, xs, us, P, d, case.mu, case.theta if theta is None else theta, mode_of(case) if mode is None else mode)
    return Sweep(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[9])


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> per instance (Sweep, total cost J of the trajectory, {alpha: (xn, un, Jn)}); the rollouts are empty for a rejection case"""
    case, s = CASES[name], start(CASES[name])
    xs, us = trajectory(case)
    out = []
    for b in range(len(case.seeds)):
        m, P = s["models"][b], s["params"][b]
        sw = sweep(case, b)
        fw = {}
        if sw.ok and not case.reject:
            d = oddp.defects(m, xs[b], us[b], P) if case.gaps == "open" else np.zeros((case.N, m.nx))
            fw = {a: oddp.forward_pass(m, s["x0"][b], xs[b], us[b], P, d, sw.K, sw.kff, a) for a in ALPHAS}
        out.append((sw, oddp.total_cost(m, xs[b], us[b], P), fw))
    return tuple(out)


def perturbed(case, b, rel, seed):
    """the case's trajectory of instance b, every entry scaled by 1 + rel x N(0, 1)"""
    xs, us = (a[b] for a in trajectory(case))
    rng = np.random.default_rng(seed)
    return xs * (1.0 + rel * rng.standard_normal(xs.shape)), us * (1.0 + rel * rng.standard_normal(us.shape))


# ---- the tolerances of one sweep and one rollout, in one place ---------------------------------------------------------------------
def gain_excess(got, ref, fraction=1.0):
    """largest |got - ref| / (fraction x (1e-7 |ref| + 1e-8 max(1, max|ref|))): <= 1 passes"""
    tol = fraction * (1e-7 * np.abs(ref) + 1e-8 * max(1.0, float(np.max(np.abs(ref)))))
    return float(np.max(np.abs(got - ref) / tol))


def spread(a, b):
    """max|a - b| / max(1, max|b|): the size of a change of the gains as the issue's table states it"""
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def assert_sweep_matches(kff, K, scal, ref, label=""):
    """one instance of DdpEngine.backward against reference()'s (Sweep, J, _); prints every figure before it asserts"""
    sw, J = ref[0], ref[1]
    eK, ek = gain_excess(K, sw.K), gain_excess(kff, sw.kff)
    print(f"{label}: K {eK:.3e} kff {ek:.3e} of the tolerance; max|K| {np.max(np.abs(sw.K)):.3e}")
    pairs = (("dV1", scal[0], sw.dV1), ("dV2", scal[1], sw.dV2), ("G1", scal[2], sw.G1), ("G2", scal[3], sw.G2), ("qu_inf", scal[6], sw.qu_inf))
    for nm, got, want in pairs:
        print(f"{label}: {nm} {got:.12e} ref {want:.12e} diff {abs(got - want):.3e} allowed {1e-8 * max(1.0, abs(want), abs(sw.dV1)):.3e}")
    print(f"{label}: J {scal[7]:.15e} ref {J:.15e} rel {abs(scal[7] - J) / abs(J):.3e}; ok {scal[4]}")
    assert sw.ok and scal[4] == 1.0, label
    assert eK <= 1.0 and ek <= 1.0, (label, eK, ek)
    for nm, got, want in pairs:
        assert abs(got - want) <= 1e-8 * max(1.0, abs(want), abs(sw.dV1)), (label, nm, got, want)
    assert abs(scal[7] - J) <= 1e-11 * abs(J), (label, scal[7], J)


def assert_rollout_matches(x, u, J, ref, alpha, label=""):
    xo, uo, Jo = ref[2][alpha]
    print(f"{label} alpha {alpha:g}: x {np.max(np.abs(x - xo)):.3e} u {np.max(np.abs(u - uo)):.3e} cost rel {abs(J - Jo) / abs(Jo):.3e}; "
          f"max|x| {np.max(np.abs(xo)):.3e} max|u| {np.max(np.abs(uo)):.3e}")
    np.testing.assert_allclose(x, xo, rtol=1e-8, atol=1e-8, err_msg=label)
    np.testing.assert_allclose(u, uo, rtol=1e-8, atol=1e-8, err_msg=label)
    assert abs(J - Jo) <= 1e-9 * abs(Jo), (label, alpha, J, Jo)


def make_engine(case):
    """a handle of the case's build with the case's trajectory loaded (needs a GPU)"""
    from srbd_horizon_amd.engine import DdpEngine
    s = start(case)
    xs, us = trajectory(case)
    consts = {k: v for k, v in s["consts"].items()}
    eng = DdpEngine(case.model, case.N, len(case.seeds), opts=options(case), consts=consts)
    if s["table"] is not None:
        eng.set_instance_consts(s["table"])
    eng.load(s["x0"], xs, us)
    return eng
