"""Non-linear user residuals compiled into the SRBD device models (srbd_horizon_amd/userterms.py, sddp_register_user_build): user
builds of srbd13 and srbd37 against the numpy oracle wrapped with the same rows (tests/user_terms_oracle.py) -- per knot, full
solves, the same rows as LinearTerm (the "_x" build) and as NonlinearTerm (a user build), the 4-wave kernel, the receding horizon
on resident data, and the builder surface end to end."""
import numpy as np
import pytest

from oracle import ddp as oddp, models as omodels
from srbd_horizon_amd import workload
from srbd_horizon_amd.ddp import DDPSolver
from srbd_horizon_amd.engine import DdpEngine, eval_knots
from tests import user_terms_defs as defs
from tests.user_terms_defs import NPB, user_case as _user_case, widen as _widen
from tests.user_terms_oracle import WithUserRows

pytestmark = pytest.mark.gpu
OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)


def _oracle(model, consts, spec):
    return WithUserRows(omodels.make_model(model, omodels.RobotConsts(**consts)), spec)


@pytest.mark.parametrize("case,model", [("srbd13_terrain", "srbd13"), ("srbd37_reach", "srbd37")])
def test_knots_of_a_user_build(case, model):
    N = 20
    spec, mid = _user_case(case, N)
    batch = workload.make_batch(model, N, [3])
    m = _oracle(model, batch["consts"], spec)
    consts = dict(batch["consts"], extra_rows=spec.extra_rows())
    P = _widen(batch["params"], spec, vary=0.2)
    rng = np.random.default_rng(4)
    ks = np.array([0, 1, 7, N - 1, N], dtype=np.int32)
    X = np.stack([m.initial_state() + 0.05 * rng.standard_normal(m.nx) for _ in ks])
    U = np.stack([m.static_input() + 0.05 * rng.standard_normal(m.nu) for _ in ks])
    Pk = np.stack([P[0, k] + 0.01 * rng.standard_normal(m.np_) * (np.arange(m.np_) >= NPB) for k in ks])
    f, F, H, g, L = eval_knots(model, N, ks, X, U, Pk, consts=consts, model_id=mid)
    fb = eval_knots(model, N, ks, X, U, Pk[:, :NPB], consts=batch["consts"])[0]
    for i, k in enumerate(ks):
        term = k == N
        Lo, lx, lu, lxx, lux, luu = m.cost_derivs(X[i], None if term else U[i], Pk[i], int(k))
        assert abs(L[i] - Lo) <= 1e-12 * max(1.0, abs(Lo)), (k, L[i], Lo)
        if term:
            np.testing.assert_allclose(g[i, :m.nx], lx, rtol=1e-11, atol=1e-11 * max(1, np.max(np.abs(lx))))
            np.testing.assert_allclose(H[i, :m.nx, :m.nx], lxx, rtol=1e-11, atol=1e-11 * np.max(np.abs(lxx)))
        else:
            np.testing.assert_array_equal(f[i], fb[i])                  # the dynamics are the base model's, bit for bit
            np.testing.assert_allclose(g[i], np.concatenate([lx, lu]), rtol=1e-11, atol=1e-11 * max(1, np.max(np.abs(lx))))
            Ho = np.block([[lxx, lux.T], [lux, luu]])
            np.testing.assert_allclose(H[i], Ho, rtol=1e-11, atol=1e-11 * np.max(np.abs(Ho)))


def _solve(model, N, batch, P, consts, mid=None, wps=1):
    eng = DdpEngine(model, N, P.shape[0], opts=dict(OPTS, waves_per_simd=wps), consts=consts, model_id=mid)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(P)
    return eng, x, u


def test_same_rows_as_linear_and_as_nonlinear_terms():
    """The same two rows declared as LinearTerm (srbd13_x) and as NonlinearTerm (a user build): the same solves."""
    N, B = 30, 256
    batch = workload.make_batch("srbd13", N, np.arange(B))
    spec, mid = _user_case("srbd13_pair", N)
    P = _widen(batch["params"], spec)
    a0 = np.zeros(19); a0[7] = 1.0; a0[0] = 0.2                           # rdot_x + 0.2 r_x - vx_ref (state row)
    a1 = np.zeros(19); a1[13 + 2] = 1.0; a1[13 + 5] = -1.0                # f0_z - f1_z (stage row)
    lin = [dict(a=a0, w=defs.PAIR_GAINS[0], kind="state"), dict(a=a1, w=defs.PAIR_GAINS[1], kind="stage")]
    el, xl, ul = _solve("srbd13", N, batch, P, dict(batch["consts"], extra_rows=lin))
    en, xn, un = _solve("srbd13", N, batch, P, dict(batch["consts"], extra_rows=spec.extra_rows()), mid)
    il, inn = el.stats["iters"], en.stats["iters"]
    differ = np.nonzero(il != inn)[0]
    print("instances with other iteration counts:", differ.tolist(), il[differ].tolist(), inn[differ].tolist())
    assert differ.size <= 2
    both = np.nonzero(el.stats["converged"].astype(bool) & en.stats["converged"].astype(bool))[0]
    assert both.size >= B - 2
    dx = np.max(np.abs(xl[both] - xn[both]), axis=(1, 2)); du = np.max(np.abs(ul[both] - un[both]), axis=(1, 2))
    dc = np.abs(el.stats["cost"][both] - en.stats["cost"][both]) / np.abs(el.stats["cost"][both])
    bad = both[(dx > 1e-6) | (du > 1e-6) | (dc > 1e-9)]
    print("converged instances that differ:", bad.tolist())
    assert bad.size == 0


@pytest.mark.parametrize("case,model,B,wps", [("srbd13_terrain", "srbd13", 32, 1), ("srbd37_reach", "srbd37", 16, 2)])
def test_solves_of_a_user_build_match_the_oracle(case, model, B, wps):
    N = 20
    spec, mid = _user_case(case, N)
    batch = workload.make_batch(model, N, np.arange(B) + 5)
    P = _widen(batch["params"], spec, vary=0.1)
    consts = dict(batch["consts"], extra_rows=spec.extra_rows())
    eng, x, u = _solve(model, N, batch, P, consts, mid, wps)
    info = eng.kernel_info()
    if model == "srbd37":                                              # the 4-wave path: every solve launch ran solve_kernel_mw
        assert info["wavefronts_per_instance"] == 4 and info["kernel"].startswith("solve_kernel_mw"), info
    else:
        assert info["wavefronts_per_instance"] == 1, info
    m = _oracle(model, batch["consts"], spec)
    iters_diff = 0
    for b in range(B):
        r = oddp.solve(m, batch["x0"][b], P[b], batch["xs"][b], batch["us"][b], oddp.DdpOptions(**OPTS))
        assert r.converged and eng.stats["converged"][b]
        assert np.max(np.abs(x[b] - r.xs)) <= 1e-6 and np.max(np.abs(u[b] - r.us)) <= 1e-6, b
        assert abs(eng.stats["cost"][b] - r.cost) <= 1e-9 * abs(r.cost), b
        iters_diff += int(eng.stats["iters"][b] != r.iters)
    assert iters_diff <= 1
    # the term acts: the plain model's solution is elsewhere
    _, x0, u0 = _solve(model, N, batch, batch["params"], batch["consts"])
    assert np.max(np.abs(x - x0)) > 1e-3


def test_receding_horizon_on_resident_data():
    """64 robots x 5 ticks through sddp_set_params / sddp_advance / sddp_solve_resident = the same ticks from host arrays; the
    user parameter columns shift with the rest"""
    N, B = 30, 64
    spec, mid = _user_case("srbd13_terrain", N)
    batch = workload.make_batch("srbd13", N, np.arange(B) + 11)
    P = _widen(batch["params"], spec, vary=0.3)
    consts = dict(batch["consts"], extra_rows=spec.extra_rows())
    dev = DdpEngine("srbd13", N, B, opts=OPTS, consts=consts, model_id=mid)
    host = DdpEngine("srbd13", N, B, opts=OPTS, consts=consts, model_id=mid)
    for e in (dev, host):
        e.load(batch["x0"], batch["xs"], batch["us"])
    dev.set_params(P)
    xd, ud = dev.solve_resident()
    xh, uh = host.solve(P)
    np.testing.assert_array_equal(xd, xh)
    for t in range(1, 5):
        last = P[:, -1].copy()
        last[:, NPB:NPB + 3] *= 1.0 + 0.05 * t                          # new terrain values enter at node N
        P = np.concatenate([P[:, 1:], last[:, None]], axis=1)
        x0 = xh[:, 1].copy()
        dev.advance(last, x0)
        xd, ud = dev.solve_resident()
        host.set_initial_state(x0)
        host.set_x_warmstart(np.concatenate([xh[:, 1:], xh[:, -1:]], axis=1))
        host.set_u_warmstart(np.concatenate([uh[:, 1:], uh[:, -1:]], axis=1))
        xh, uh = host.solve(P)
        np.testing.assert_array_equal(dev.stats["iters"], host.stats["iters"])
        np.testing.assert_array_equal(xd, xh)
        np.testing.assert_array_equal(ud, uh)


def test_example_problem_through_the_adapter():
    ex = defs.example_module()
    ns = 20
    pb, prb = ex.build_problem(ns)
    solver = DDPSolver(prb, ex.OPTS)
    solver.setInitialState(pb.getInitialState())
    solver.set_u_warmstart(np.repeat(pb.getStaticInput()[:, None], ns, axis=1))
    assert solver.solve()
    sol = solver.getSolutionDict()
    names = [v.getName() for v in prb.var_container.getVarList(offset=False)]
    assert set(sol) == set(names) | {"x_opt", "u_opt"}
    assert sol["x_opt"].shape == (37, ns + 1) and sol["u_opt"].shape == (24, ns)
    # the gain is runtime data: another value, the same build, another solution
    prb.function_container.getCost()["reach"].term.gain = 1e4
    s2 = DDPSolver(prb, ex.OPTS)
    assert s2.ddp_solver.model_id == solver.ddp_solver.model_id
    s2.setInitialState(pb.getInitialState())
    s2.set_u_warmstart(np.repeat(pb.getStaticInput()[:, None], ns, axis=1))
    assert s2.solve()
    assert np.max(np.abs(s2.getSolutionDict()["x_opt"] - sol["x_opt"])) > 1e-6
