"""GPU parity tests proper: the HIP engine (through the C ABI) vs the float64 CPU oracle on the same seeded inputs.

Tolerances (floating point, fp64 on both sides; BASELINE.json target is <= 1e-4 l-inf on trajectories):
  per-knot model evaluation   rtol 1e-11 (same formulas, different operation order / FMA contraction)
  one backward sweep          gains rtol 1e-8  (30 dependent 13x13 Riccati steps, cond ~1e6)
  one forward pass            1e-9
  converged solves            l-inf(x,u) <= 1e-6, relative cost <= 1e-9, same iteration count
"""
import numpy as np
import pytest

from oracle import ddp as oddp
from oracle import models as omodels
from srbd_horizon_amd import workload
from srbd_horizon_amd.engine import DdpEngine, eval_knots
from tests import options_cases as oc, parity

pytestmark = pytest.mark.gpu

MODELS = ["srbd13", "srbd37", "lip30", "srbd61"]
SOLVED = [("srbd13", 30), ("srbd37", 20), ("lip30", 20), ("srbd61", 20)]      # model, N of the whole-solve and one-sweep tests


def _oracle_model(name, consts=None):
    cst = omodels.RobotConsts()
    for k, v in (consts or {}).items():
        if hasattr(cst, k):
            setattr(cst, k, v)
    return omodels.make_model(name, cst)


def _opts(**over):
    return dict(oc.BASE, **over)      # dsrbd_example.py:55-58


def _engine_consts(name, batch):
    """srbd61's handles are built with the workload's explicit constants (tests/test_gpu_srbd61.py checks that the defaults are the same
    robot); the other models' with the defaults"""
    return batch["consts"] if name == "srbd61" else None


def _oracle_opts(**over):
    return oddp.DdpOptions(**_opts(**over))


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("imode,lever", [(0, 1.0), (1, -1.0)])
def test_eval_knots_matches_oracle(name, imode, lever):
    if name == "lip30" and imode == 1:
        pytest.skip("LIP has no inertia")
    N = 20
    m = _oracle_model(name, dict(inertia_mode=imode, lever_sign=lever))
    rng = np.random.default_rng(5)
    ks = np.array([0, 1, 7, N - 1, N, 3, N, 0], dtype=np.int32)
    nk = len(ks)
    X = np.tile(m.initial_state(), (nk, 1)) + 0.05 * rng.standard_normal((nk, m.nx))
    U = np.tile(m.static_input(), (nk, 1)) + 0.05 * rng.standard_normal((nk, m.nu))
    P = np.tile(m.default_params(N)[3], (nk, 1)) + 0.05 * rng.standard_normal((nk, m.np_))
    consts = dict(inertia_mode=imode, lever_sign=lever)
    if name == "srbd61":
        consts["feet"] = m.cst.feet8[:4]
    f, F, H, g, L = eval_knots(name, N, ks, X, U, P, consts=consts)
    for t, k in enumerate(ks):
        if k < N:
            np.testing.assert_allclose(f[t], m.f(X[t], U[t], P[t]), rtol=1e-12, atol=1e-13)
            fx, fu = m.f_jac(X[t], U[t], P[t])
            np.testing.assert_allclose(F[t], np.hstack([fx, fu]), rtol=1e-11, atol=1e-12)
            Lo, lx, lu, lxx, lux, luu = m.cost_derivs(X[t], U[t], P[t], int(k))
            Ho = np.block([[lxx, lux.T], [lux, luu]])
            go = np.concatenate([lx, lu])
        else:
            Lo, lx, _, lxx, _, _ = m.cost_derivs(X[t], None, P[t], int(k))
            Ho = np.zeros((m.nx + m.nu,) * 2); Ho[:m.nx, :m.nx] = lxx
            go = np.concatenate([lx, np.zeros(m.nu)])
        assert abs(L[t] - Lo) <= 1e-12 * max(1.0, abs(Lo))
        np.testing.assert_allclose(g[t], go, rtol=1e-11, atol=1e-11 * max(1.0, np.max(np.abs(go))))
        np.testing.assert_allclose(H[t], Ho, rtol=1e-11, atol=1e-11 * max(1.0, np.max(np.abs(Ho))))


@pytest.mark.parametrize("name,N", SOLVED)
def test_backward_and_forward_pass_match_oracle(name, N):
    seeds = [0, 5, 13]
    batch = workload.make_batch(name, N, seeds)
    m = _oracle_model(name)
    rng = np.random.default_rng(1)
    xs = batch["xs"] + 1e-3 * rng.standard_normal(batch["xs"].shape)       # open gaps: multiple shooting
    us = batch["us"] + 1e-3 * rng.standard_normal(batch["us"].shape)
    xs[:, 0] = batch["x0"]
    eng = DdpEngine(name, N, len(seeds), opts=_opts(), consts=_engine_consts(name, batch))
    eng.load(batch["x0"], xs, us)
    kff, K, scal = eng.backward(batch["params"], mu=0.0)
    xg, ug, Jg = eng.forward(batch["params"], 0.25)
    for b in range(len(seeds)):
        P = batch["params"][b]
        d = oddp.defects(m, xs[b], us[b], P)
        ok, Ko, ko, dV1, dV2, G1, G2, Vx0, Vxx0, qu = oddp.backward_pass(m, xs[b], us[b], P, d, 0.0)
        assert ok and scal[b, 4] == 1.0
        sK = max(1.0, np.max(np.abs(Ko)))
        np.testing.assert_allclose(K[b], Ko, rtol=1e-7, atol=1e-8 * sK)
        np.testing.assert_allclose(kff[b], ko, rtol=1e-7, atol=1e-8 * max(1.0, np.max(np.abs(ko))))
        for got, ref in ((scal[b, 0], dV1), (scal[b, 1], dV2), (scal[b, 2], G1), (scal[b, 3], G2)):
            assert abs(got - ref) <= 1e-8 * max(1.0, abs(ref), abs(dV1))
        assert abs(scal[b, 7] - oddp.total_cost(m, xs[b], us[b], P)) <= 1e-11 * abs(scal[b, 7])
        xo, uo, Jo = oddp.forward_pass(m, batch["x0"][b], xs[b], us[b], P, d, Ko, ko, 0.25)
        np.testing.assert_allclose(xg[b], xo, rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(ug[b], uo, rtol=1e-8, atol=1e-8)
        assert abs(Jg[b] - Jo) <= 1e-9 * abs(Jo)


@pytest.mark.parametrize("name,N", SOLVED)
def test_converged_solve_matches_oracle(name, N):
    """Multiple-shooting solves to convergence (options of dsrbd_example.py:55-58).  Seeds 0,1,6,16 converge in 8-18
    Gauss-Newton iterations on srbd13 (commanded-velocity seeds need up to 100)."""
    seeds = [0, 1, 6, 16]
    batch = workload.make_batch(name, N, seeds)
    m = _oracle_model(name)
    eng = DdpEngine(name, N, len(seeds), opts=_opts(), consts=_engine_consts(name, batch))
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    st = eng.stats
    conv = eng.is_converged()
    for b in range(len(seeds)):
        r = oddp.solve(m, batch["x0"][b], batch["params"][b], batch["xs"][b], batch["us"][b], _oracle_opts())
        assert r.converged and conv[b] and st["converged"][b] and st["status"][b] == 0
        parity.assert_matches_numpy_oracle(x[b], u[b], st[b], r, b)


def test_single_shooting_start_matches_oracle():
    """initial_rollout=1: the x warm start is ignored, the start is an open-loop rollout of u (unstable for this
    inverted-pendulum-like system unless u is close to a solution: warm start u from a converged solve, perturbed)."""
    N, seeds = 30, [0, 6]
    batch = workload.make_batch("srbd13", N, seeds)
    m = _oracle_model("srbd13")
    eng = DdpEngine("srbd13", N, len(seeds), opts=_opts())
    eng.load(batch["x0"], batch["xs"], batch["us"])
    _, u0 = eng.solve(batch["params"])
    u0 = u0 + 1e-3 * np.random.default_rng(0).standard_normal(u0.shape)
    eng.set_options(initial_rollout=1)
    eng.set_u_warmstart(u0)
    x, u = eng.solve(batch["params"])
    for b in range(len(seeds)):
        o = _oracle_opts()
        o.initial_rollout = True
        r = oddp.solve(m, batch["x0"][b], batch["params"][b], batch["xs"][b], u0[b], o)
        assert r.converged and eng.stats["converged"][b]
        assert eng.stats["iters"][b] == r.iters
        assert eng.stats["gap"][b] == 0.0
        assert np.max(np.abs(x[b] - r.xs)) <= 1e-6 and np.max(np.abs(u[b] - r.us)) <= 1e-6


def test_iteration_by_iteration_trace_matches_oracle():
    """max_iters = 1, 2, 3: the engine and the oracle agree after every iteration, not only at convergence."""
    N, seeds = 30, [4]
    batch = workload.make_batch("srbd13", N, seeds)
    m = _oracle_model("srbd13")
    for it in (1, 2, 3):
        eng = DdpEngine("srbd13", N, 1, opts=_opts(max_iters=it, cost_reduction_ths=1e-12))
        eng.load(batch["x0"], batch["xs"], batch["us"])
        x, u = eng.solve(batch["params"])
        r = oddp.solve(m, batch["x0"][0], batch["params"][0], batch["xs"][0], batch["us"][0],
                       _oracle_opts(max_iters=it, cost_reduction_ths=1e-12))
        assert eng.stats["iters"][0] == r.iters == it
        assert eng.stats["alpha"][0] == r.alpha
        assert np.max(np.abs(x[0] - r.xs)) <= 1e-8 and np.max(np.abs(u[0] - r.us)) <= 1e-8
        assert abs(eng.stats["cost"][0] - r.cost) <= 1e-10 * abs(r.cost)
        eng.close()


@pytest.mark.parametrize("model,N", SOLVED)
def test_regularisation_bump_on_indefinite_quu(model, N):
    """mu0 < 0 large makes Quu indefinite: the engine must bump mu (ddp.py:34-35) exactly like the oracle.  On the 4-wavefront
    kernel (srbd37, lip30; srbd61 in its W-free layout: the gains over GC | WC) a failed sweep leaves tiles that alias each other
    half-written: the retry must not see them."""
    seeds = [3]
    batch = workload.make_batch(model, N, seeds)
    m = _oracle_model(model)
    over = dict(mu0=-1e9, max_iters=3)
    eng = DdpEngine(model, N, 1, opts=_opts(**over), consts=_engine_consts(model, batch))
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    r = oddp.solve(m, batch["x0"][0], batch["params"][0], batch["xs"][0], batch["us"][0], _oracle_opts(**over))
    assert eng.stats["mu"][0] == pytest.approx(r.mu, rel=1e-12)
    assert eng.stats["iters"][0] == r.iters
    assert np.max(np.abs(x[0] - r.xs)) <= 1e-7


def test_backtracking_line_search_picks_the_same_alpha():
    """Commanded-velocity seeds need alpha < 1 in the first iterations (oracle: 0.125 / 0.25): the one-pass parallel
    ladder must select exactly what sequential backtracking selects, iteration after iteration."""
    N = 30
    m = _oracle_model("srbd13")
    seen = set()
    for seed in (7, 2):
        batch = workload.make_batch("srbd13", N, [seed])
        for it in (1, 2, 3, 8):
            over = dict(max_iters=it, cost_reduction_ths=1e-12)
            eng = DdpEngine("srbd13", N, 1, opts=_opts(**over))
            eng.load(batch["x0"], batch["xs"], batch["us"])
            x, u = eng.solve(batch["params"])
            r = oddp.solve(m, batch["x0"][0], batch["params"][0], batch["xs"][0], batch["us"][0], _oracle_opts(**over))
            assert eng.stats["iters"][0] == r.iters == it
            assert eng.stats["alpha"][0] == r.alpha
            seen.add(r.alpha)
            assert np.max(np.abs(x[0] - r.xs)) <= 1e-7 and np.max(np.abs(u[0] - r.us)) <= 1e-7
            assert abs(eng.stats["cost"][0] - r.cost) <= 1e-10 * abs(r.cost)
            eng.close()
    assert min(seen) < 1.0, "test input does not exercise backtracking"


def test_exhausted_line_search_stops_with_status_4():
    """alpha falling below alpha_converge_threshold stops the solve; with open gaps / a predicted decrease left
    that is a stall (status 4, not converged), not an optimum."""
    N = 30
    batch = workload.make_batch("srbd13", N, [7])
    m = _oracle_model("srbd13")
    over = dict(alpha_converge_threshold=0.5, max_iters=5)        # seed 7 needs alpha = 0.125 in iteration 1
    eng = DdpEngine("srbd13", N, 1, opts=_opts(**over))
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    r = oddp.solve(m, batch["x0"][0], batch["params"][0], batch["xs"][0], batch["us"][0], _oracle_opts(**over))
    assert r.iters == 0 and not r.converged and r.status == 4 and r.alpha == 0.0
    assert eng.stats["iters"][0] == 0 and eng.stats["converged"][0] == 0 and eng.stats["status"][0] == 4 and eng.stats["alpha"][0] == 0.0
    assert not eng.is_converged()[0]
    np.testing.assert_array_equal(x[0], batch["xs"][0]); np.testing.assert_array_equal(u[0], batch["us"][0])


def test_exhausted_line_search_at_an_optimum_is_status_0():
    """`converged = 1` always comes with `status = 0`.  Restart from the optimum with an Armijo fraction nothing can
    meet: the first sweep still predicts a (tiny) decrease above cost_reduction_ths, so the regular exit does not fire, the
    whole ladder is rolled out and rejected, and the RELATIVE test expected <= ths * max(1, |J|) (include/sddp.h, sddp_stats)
    declares the point optimal: status 0, converged, no iteration, one rollout pass.  With a threshold that test cannot meet
    either, the same call is a stall: status 4, not converged."""
    N = 30
    batch = workload.make_batch("srbd13", N, [7])
    m = _oracle_model("srbd13")
    eng = DdpEngine("srbd13", N, 1, opts=_opts())
    eng.load(batch["x0"], batch["xs"], batch["us"])
    xo, uo = eng.solve(batch["params"])
    assert eng.stats["status"][0] == 0 and eng.stats["converged"][0] == 1
    for ths, status, conv in ((1e-12, 0, 1), (1e-30, 4, 0)):
        over = dict(max_iters=5, alpha_converge_threshold=0.5, beta=1e6, cost_reduction_ths=ths)
        e2 = DdpEngine("srbd13", N, 1, opts=_opts(**over))
        e2.load(batch["x0"], xo, uo)
        x2, u2 = e2.solve(batch["params"])
        st = e2.stats
        r = oddp.solve(m, batch["x0"][0], batch["params"][0], xo[0], uo[0], _oracle_opts(**over))
        assert st["expected"][0] >= ths and st["rollouts"][0] >= 1 and st["iters"][0] == 0       # the line search did run, and failed
        assert (st["status"][0], st["converged"][0]) == (status, conv) == (r.status, int(r.converged)), (ths, st, r.status)
        assert bool(e2.is_converged()[0]) == bool(conv)
        np.testing.assert_array_equal(x2, xo); np.testing.assert_array_equal(u2, uo)             # nothing was accepted


def test_full_size_batch_properties():
    """BASELINE config 3 size (B = 1024, N = 30): size-independent properties + spot parity on a few instances."""
    N, B = 30, 1024
    batch = workload.make_batch("srbd13", N, np.arange(B))
    eng = DdpEngine("srbd13", N, B, opts=_opts())
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    st = eng.stats.copy()
    assert np.all((st["status"] == 0) | (st["status"] == 1) | (st["status"] == 4))     # converged, max_iters or stalled, never a failure
    assert np.all(st["converged"][st["status"] == 0] == 1) and np.all(st["converged"][st["status"] == 1] == 0)
    assert np.mean(st["converged"]) > 0.8
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u)) and np.all(np.isfinite(st["cost"]))
    np.testing.assert_array_equal(x[:, 0], batch["x0"])                     # x_0 is pinned
    assert np.all(st["gap"][st["converged"] == 1] <= 1e-9)                  # converged => multiple-shooting gaps closed
    m = _oracle_model("srbd13")
    for b in range(0, B, 97):
        # dynamic feasibility and reported cost, checked with the ORACLE's f and L on the returned trajectory
        d = oddp.defects(m, x[b], u[b], batch["params"][b])
        assert abs(np.sum(np.abs(d)) - st["gap"][b]) <= 1e-9 * max(1.0, st["gap"][b])
        assert abs(oddp.total_cost(m, x[b], u[b], batch["params"][b]) - st["cost"][b]) <= 1e-9 * st["cost"][b]
        # the solve never increases the merit: final cost below the cost of the feasibilised start
        assert st["cost"][b] < oddp.total_cost(m, batch["xs"][b], batch["us"][b], batch["params"][b]) * 10
    # near-idempotence: re-solving a converged instance from its solution never raises the cost and barely moves it
    # (Gauss-Newton converges linearly here, so a restart may still take a few tiny steps)
    eng.set_x_warmstart(x); eng.set_u_warmstart(u)
    x2, u2 = eng.solve(batch["params"])
    done = st["converged"] == 1
    assert np.all(eng.stats["cost"][done] <= st["cost"][done] * (1 + 1e-12))
    assert np.all(eng.stats["cost"][done] >= st["cost"][done] * (1 - 1e-8))
    assert np.max(np.abs(x2[done] - x[done])) <= 1e-3
    # batch independence: instance b solved alone gives bit-identical output
    for b in (0, 511, 1023):
        e1 = DdpEngine("srbd13", N, 1, opts=_opts())
        e1.load(batch["x0"][b:b + 1], batch["xs"][b:b + 1], batch["us"][b:b + 1])
        x1, u1 = e1.solve(batch["params"][b:b + 1])
        np.testing.assert_array_equal(x1[0], x[b]); np.testing.assert_array_equal(u1[0], u[b])
        e1.close()
    # spot parity against the oracle at the BASELINE tolerance (1e-4 l-inf)
    for b in (0, 6, 16, 19):
        r = oddp.solve(m, batch["x0"][b], batch["params"][b], batch["xs"][b], batch["us"][b], _oracle_opts())
        assert st["iters"][b] == r.iters
        assert np.max(np.abs(x[b] - r.xs)) <= 1e-4 and np.max(np.abs(u[b] - r.us)) <= 1e-4
        assert abs(st["cost"][b] - r.cost) <= 1e-6 * abs(r.cost)


def test_receding_horizon_loop_runs_and_tracks():
    """mpc.MpcLoop = the body of dsrbd_example.py:82-185 without ROS: a few walking ticks on the reference-faithful model
    (ns = 20, T = 1 s as in dsrbd_example.py:30-31) and on the metric model."""
    from srbd_horizon_amd.mpc import MpcLoop
    for model, ns in (("srbd37", 20), ("srbd13", 30), ("lip30", 20)):
        loop = MpcLoop(model, ns)
        flags = loop.run(6, motion="walking", axes=(1.0, 0.0))
        sol = loop.solver.getSolutionDict()
        assert sol["x_opt"].shape == (loop.solver.state_size, ns + 1) and sol["u_opt"].shape == (loop.solver.input_size, ns)
        assert np.all(np.isfinite(loop.state))
        if model == "lip30":                                          # dlip_example.py:89-160
            assert set(["r", "rdot", "z", "c0", "c3", "cddot0"]).issubset(sol.keys()) and sol["z"].shape == (3, ns)
        else:
            assert set(["r", "o", "rdot", "w", "f0", "f1"]).issubset(sol.keys())
            assert sol["r"].shape == (3, ns + 1) and sol["f0"].shape == (3, ns)
            assert abs(np.linalg.norm(loop.state[3:7]) - 1.0) < 1e-12
        assert len(loop.solve_ms) == 6 and all(np.isfinite(loop.solve_ms))
        assert loop.wpg.step_counter == 6
        assert abs(loop.state[2] - 0.88) < 0.05                       # CoM height is tracked
        np.testing.assert_allclose(sol["x_opt"][:, 0], loop.solver._x0[0], atol=0)   # node 0 is the measured state
        rec = loop.reference_record(sol)                              # what cartesio.py:58-79 publishes, without ROS
        np.testing.assert_array_equal(rec["com"], sol["r"][:, 1])
        np.testing.assert_array_equal(rec["base_link"], sol["o"][:, 1] if "o" in sol else [0.0, 0.0, 0.0, 1.0])
        assert set(rec["contacts"]) == {"left_sole_link", "right_sole_link"}
        if model in ("srbd37", "lip30"):                              # line foot: midpoint of its two contact points
            np.testing.assert_allclose(rec["contacts"]["left_sole_link"], 0.5 * (sol["c0"][:, 1] + sol["c1"][:, 1]), atol=0)
            np.testing.assert_allclose(rec["contacts"]["right_sole_link"], 0.5 * (sol["c2"][:, 1] + sol["c3"][:, 1]), atol=0)


def test_closed_loop_walks_for_a_hundred_ticks():
    """The loop bench.py times as ms/MPC-tick is a robot that actually walks: 120 closed-loop ticks (solve -> first input ->
    simulator step) with a forward command.  The CoM advances at the commanded 0.5 m/s, stays at height and on its line; every
    tick converges in a handful of iterations.  (Round 1's srbd13 loop never moved its footstep plan -- the metric model's
    contacts are data -- and the CoM left the feet behind: z = 5 m after 80 ticks, with every solve still 'converged'.)"""
    from srbd_horizon_amd.mpc import MpcLoop
    for model, ns in (("srbd13", 30), ("srbd37", 20), ("lip30", 20)):
        loop = MpcLoop(model, ns, warm_start="device")
        its, xs = [], []
        for t in range(120):
            ok, _ = loop.tick("walking", (1.0, 0.0))
            assert ok
            its.append(int(loop.solver.stats["iters"]))
            xs.append(loop.state[0])
        v = (xs[-1] - xs[59]) / (60 * 0.05)                           # mean forward velocity over the last 3 s
        assert 0.3 < v < 0.6, (model, v)                              # command: 0.5 m/s (dsrbd_example.py:112, :119-122)
        assert abs(loop.state[1]) < 0.1 and 0.8 < loop.state[2] < 1.1, (model, loop.state[:3])
        assert max(its[5:]) <= 8, (model, max(its))


def test_closed_loop_tracking_holds_under_a_per_tick_iteration_budget():
    """The real-time remedy for a slow tick (bench.py ms_per_fleet_tick.budgeted): at most `max_iters` DDP
    iterations per tick, the unfinished iterate (status 1) is carried on as the next tick's warm start -- the solver object keeps
    its previous solution (dsrbd_example.py:59).  Closed loop, walking at the commanded 0.5 m/s: the budgeted loop must track
    like the loop that solves every tick to convergence."""
    from srbd_horizon_amd.mpc import MpcLoop, EXAMPLE_OPTS
    for model, ns, budget in (("srbd13", 30, 2), ("srbd37", 20, 2)):
        full = MpcLoop(model, ns, warm_start="device")
        bud = MpcLoop(model, ns, warm_start="device", opts=dict(EXAMPLE_OPTS, max_iters=budget))
        xs_f, xs_b, unfinished, its = [], [], 0, []
        for t in range(100):
            full.tick("walking", (1.0, 0.0))
            ok, _ = bud.tick("walking", (1.0, 0.0))
            st = bud.solver.stats
            assert int(st["iters"]) <= budget and int(st["status"]) in (0, 1)
            unfinished += int(st["status"]) == 1
            its.append(int(st["iters"]))
            xs_f.append(full.state.copy()); xs_b.append(bud.state.copy())
        xs_f, xs_b = np.array(xs_f), np.array(xs_b)
        assert unfinished >= 5, (model, unfinished)                                   # the budget did bind
        v = (xs_b[-1, 0] - xs_b[39, 0]) / (60 * 0.05)                                 # mean forward velocity over the last 3 s
        assert 0.3 < v < 0.6, (model, v)
        assert abs(xs_b[-1, 1]) < 0.1 and 0.8 < xs_b[-1, 2] < 1.1, (model, xs_b[-1, :3])
        dev = np.max(np.abs(xs_b[:, 0:3] - xs_f[:, 0:3]))                             # CoM path against the converged loop
        print(f"{model}: budget {budget} iterations/tick, {unfinished} of 100 ticks unfinished, CoM deviation from the converged loop {dev:.2e} m")
        assert dev < 0.02, (model, dev)


def test_whole_bench_batch_matches_the_c_oracle(record_property):
    """All 1024 instances of the bench batch (BASELINE configs[2]) against the plain-C restatement of the oracle
    (oracle/c, pinned to the numpy oracle by tests/test_oracle_c.py): same iteration count and, at the north_star tolerance
    (1e-4 l-inf), the same trajectory -- stragglers included (up to 93 iterations, step lengths down to 2^-9, i.e. the
    line-search path whose winner is not one of the kept candidates).  An instance on another path is explained step by step
    (tests/shadow.py); the full set of instances bench.py times is tests/test_gpu_divergence.py."""
    from tests import shadow
    from tests.shadow import assert_batch
    N, B = 30, 1024
    batch = workload.make_batch("srbd13", N, np.arange(B))
    res = shadow.check_batch("srbd13", N, batch, dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), {},
                             omodels.RobotConsts(**batch["consts"]), threads=8)
    st = res["st"]
    assert st["iters"].max() >= 60 and st["rollouts"].max() > st["iters"].max()       # the fallback path did run
    assert_batch(res, "bench_batch_1024", record_property)


@pytest.mark.parametrize("name,N,B", [("srbd13", 1, 3), ("srbd13", 2, 1), ("srbd13", 100, 2), ("lip30", 1, 2), ("srbd37", 2, 2),
                                      ("lip30", 70, 1)])
def test_extreme_horizons_and_ragged_batches(name, N, B):
    """Shortest horizons, a horizon longer than a wavefront (the lane-per-knot phases wrap), odd batch sizes."""
    batch = workload.make_batch(name, N, np.arange(B) + 3)
    eng = DdpEngine(name, N, B, opts=_opts())
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    st = eng.stats.copy()
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u))
    m = _oracle_model(name)
    for b in range(B):
        r = oddp.solve(m, batch["x0"][b], batch["params"][b], batch["xs"][b], batch["us"][b], _oracle_opts())
        assert st["iters"][b] == r.iters and bool(st["converged"][b]) == r.converged
        assert np.max(np.abs(x[b] - r.xs)) <= 1e-6 and np.max(np.abs(u[b] - r.us)) <= 1e-6
        assert abs(st["cost"][b] - r.cost) <= 1e-9 * max(1.0, abs(r.cost))


BARRIER = dict(friction_barrier_weight=6.0, friction_barrier_sharpness=30.0, friction_cone_coefficient=0.8)


@pytest.mark.parametrize("name", ["srbd13", "srbd37", "srbd61"])
def test_friction_cone_barrier_knots_match_oracle(name):
    """SURVEY 8(f) item 3 -- the inequality handling the reference disables (prb.py:172-177, ddp.py:197-202), as an opt-in
    exponential barrier on the contact forces: per-knot value, gradient and Gauss-Newton Hessian of the barrier builds."""
    N = 20
    m = _oracle_model(name, BARRIER)
    rng = np.random.default_rng(9)
    ks = np.array([0, 1, 7, N - 1, N], dtype=np.int32)
    nk = len(ks)
    X = np.tile(m.initial_state(), (nk, 1)) + 0.05 * rng.standard_normal((nk, m.nx))
    U = np.tile(m.static_input(), (nk, 1)) + 0.05 * rng.standard_normal((nk, m.nu))
    P = np.tile(m.default_params(N)[3], (nk, 1)) + 0.05 * rng.standard_normal((nk, m.np_))
    f, F, H, g, L = eval_knots(name, N, ks, X, U, P, consts=BARRIER)
    f0, F0, H0, g0, L0 = eval_knots(name, N, ks, X, U, P)
    assert np.all(L[:-1] > L0[:-1]) and L[-1] == L0[-1]                  # stage nodes carry the barrier, the terminal node not
    np.testing.assert_array_equal(f, f0)
    for t, k in enumerate(ks[:-1]):
        Lo, lx, lu, lxx, lux, luu = m.cost_derivs(X[t], U[t], P[t], int(k))
        Ho = np.block([[lxx, lux.T], [lux, luu]])
        go = np.concatenate([lx, lu])
        assert abs(L[t] - Lo) <= 1e-12 * max(1.0, abs(Lo))
        np.testing.assert_allclose(g[t], go, rtol=1e-11, atol=1e-11 * max(1.0, np.max(np.abs(go))))
        np.testing.assert_allclose(H[t], Ho, rtol=1e-11, atol=1e-11 * max(1.0, np.max(np.abs(Ho))))


@pytest.mark.parametrize("name,N", [("srbd13", 30), ("srbd37", 20), ("srbd61", 12)])
def test_friction_cone_barrier_solve_matches_oracle_and_tightens_the_cone(name, N):
    seeds = [0, 1, 6]
    batch = workload.make_batch(name, N, seeds)
    m = _oracle_model(name, BARRIER)
    res = {}
    for tag, consts in (("off", dict(batch["consts"])), ("on", dict(batch["consts"], **BARRIER))):
        eng = DdpEngine(name, N, len(seeds), opts=_opts(), consts=consts)
        eng.load(batch["x0"], batch["xs"], batch["us"])
        x, u = eng.solve(batch["params"])
        res[tag] = (x, u, eng.stats.copy())
    x, u, st = res["on"]
    for b in range(len(seeds)):
        r = oddp.solve(m, batch["x0"][b], batch["params"][b], batch["xs"][b], batch["us"][b], _oracle_opts())
        assert st["iters"][b] == r.iters and bool(st["converged"][b]) == r.converged
        assert np.max(np.abs(x[b] - r.xs)) <= 1e-6 and np.max(np.abs(u[b] - r.us)) <= 1e-6
        assert abs(st["cost"][b] - r.cost) <= 1e-9 * abs(r.cost)
    # worst violation of the linearised cone A f <= 0 over all knots and contacts shrinks when the barrier is on
    A = omodels.friction_cone_rows(0.8)
    fcols = [slice(3 * i, 3 * i + 3) for i in range(2)] if name == "srbd13" else [slice(6 * i + 3, 6 * i + 6) for i in range(4 if name == "srbd37" else 8)]
    viol = {t: max(float(np.max(res[t][1][..., c] @ A.T)) for c in fcols) for t in res}
    assert viol["on"] < viol["off"] or viol["off"] <= 0.0, viol
    with pytest.raises(RuntimeError, match="friction"):
        DdpEngine(name, N, 1, consts=dict(friction_barrier_weight=-1.0))
    if name == "srbd61":          # lower / upper hold 64 entries of z, this model has 109: friction-cone barrier only
        with pytest.raises(RuntimeError, match="bound barrier"):
            DdpEngine(name, N, 1, consts=dict(bound_barrier_weight=1.0))


@pytest.mark.parametrize("name,N,seeds", [("srbd13", 30, [0, 1, 2, 4, 6]), ("srbd37", 20, [3, 5, 12])])
def test_full_second_order_mode_matches_oracle(name, N, seeds):
    """second_order = 2 ("full DDP": v'.f_zz for the wdot and quaternion rows + exact Hessian of the wdot residual, after full
    steps, Gauss-Newton fallback): the SO2 kernel builds against the numpy oracle, iteration by iteration."""
    batch = workload.make_batch(name, N, seeds)
    m = _oracle_model(name)
    eng = DdpEngine(name, N, len(seeds), opts=_opts(second_order=2))
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    st = eng.stats.copy()
    differs = 0
    for b in range(len(seeds)):
        r = oddp.solve(m, batch["x0"][b], batch["params"][b], batch["xs"][b], batch["us"][b], _oracle_opts(second_order=2))
        r1 = oddp.solve(m, batch["x0"][b], batch["params"][b], batch["xs"][b], batch["us"][b], _oracle_opts(second_order=1))
        assert st["iters"][b] == r.iters and bool(st["converged"][b]) == r.converged and st["alpha"][b] == r.alpha
        assert np.max(np.abs(x[b] - r.xs)) <= 1e-6 and np.max(np.abs(u[b] - r.us)) <= 1e-6
        assert abs(st["cost"][b] - r.cost) <= 1e-9 * abs(r.cost)
        differs += int(r.iters != r1.iters)
    # the mode does take another path than the default one.  (srbd37: of the seeds 0..31 only 12 takes another number of iterations,
    # 7 against 6; term by term the second_order = 2 builds are compared in tests/test_gpu_sweep_modes.py)
    assert differs > 0
    with pytest.raises(RuntimeError):
        eng.set_options(second_order=1)                   # another kernel build and record size: create-time choice


@pytest.mark.parametrize("name,N,consts", [("srbd13", 30, dict(inertia_mode=1)), ("srbd13", 4, dict(inertia_mode=1, lever_sign=-1.0)),
                                           ("srbd13", 2, {}), ("srbd13", 1, {}), ("srbd37", 3, dict(inertia_mode=1)),
                                           ("srbd13", 30, dict(friction_barrier_weight=2.0, friction_barrier_sharpness=4.0)),
                                           ("srbd37", 10, dict(friction_barrier_weight=2.0, friction_barrier_sharpness=4.0))])
def test_full_second_order_mode_other_constants_and_short_horizons(name, N, consts):
    """second_order = 2 with the physical inertia rotation R I R^T / the other lever-arm sign (the second derivatives of I_w take
    another branch), on horizons of one to four knots, and together with the opt-in friction-cone barrier (whose exact Hessian is
    twice its Gauss-Newton one)."""
    seeds = [2, 9]
    batch = workload.make_batch(name, N, seeds)
    m = _oracle_model(name, consts)
    eng = DdpEngine(name, N, len(seeds), opts=_opts(second_order=2), consts=dict(batch["consts"], **consts))
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    for b in range(len(seeds)):
        r = oddp.solve(m, batch["x0"][b], batch["params"][b], batch["xs"][b], batch["us"][b], _oracle_opts(second_order=2))
        assert eng.stats["iters"][b] == r.iters and bool(eng.stats["converged"][b]) == r.converged
        assert np.max(np.abs(x[b] - r.xs)) <= 1e-6 and np.max(np.abs(u[b] - r.us)) <= 1e-6
        assert abs(eng.stats["cost"][b] - r.cost) <= 1e-9 * abs(r.cost)


@pytest.mark.parametrize("name,N,consts,so", [("srbd13", 30, dict(inertia_mode=1), 1), ("srbd13", 30, dict(inertia_mode=1), 0),
                                              ("srbd37", 20, dict(inertia_mode=1), 1), ("srbd13", 6, dict(lever_sign=-1.0), 1)])
def test_converged_solves_with_the_optional_model_conventions(name, N, consts, so):
    """The two upstream-unverified conventions as options: physical inertia rotation R I R^T instead of the
    reference's element-wise product, and the other lever-arm sign -- whole solves against the numpy oracle."""
    seeds = [1, 5, 8]
    batch = workload.make_batch(name, N, seeds)
    m = _oracle_model(name, consts)
    eng = DdpEngine(name, N, len(seeds), opts=_opts(second_order=so), consts=dict(batch["consts"], **consts))
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"])
    for b in range(len(seeds)):
        r = oddp.solve(m, batch["x0"][b], batch["params"][b], batch["xs"][b], batch["us"][b], _oracle_opts(second_order=so))
        assert eng.stats["iters"][b] == r.iters and bool(eng.stats["converged"][b]) == r.converged and eng.stats["status"][b] == r.status
        if r.converged:
            assert np.max(np.abs(x[b] - r.xs)) <= 1e-6 and np.max(np.abs(u[b] - r.us)) <= 1e-6
            assert abs(eng.stats["cost"][b] - r.cost) <= 1e-9 * abs(r.cost)


def test_full_second_order_whole_batch_iteration_histogram(record_property):
    """The bench batch in second_order = 2 against the C oracle (same mode): end-to-end parity on the same path, every accepted GPU
    step shadowed on the others (tests/shadow.py, as tests/test_gpu_divergence.py does for the default mode); prints the iteration
    histogram DESIGN.md quotes."""
    from tests import shadow
    from tests.shadow import assert_batch
    N, B = 30, 1024
    batch = workload.make_batch("srbd13", N, np.arange(B))
    res = shadow.check_batch("srbd13", N, batch, _opts(second_order=2), {}, omodels.RobotConsts(**batch["consts"]), threads=8)
    st, it = res["st"], res["st"]["iters"]
    print(f"second_order=2: GPU iterations mean {it.mean():.2f} median {np.median(it):.0f} p90 {np.percentile(it, 90):.0f} "
          f"p99 {np.percentile(it, 99):.0f} max {it.max()}; converged {st['converged'].mean():.4f}; "
          f"{len(res['explained'])} instances differ from the C oracle in iteration count (the two CPU builds: {res['n_cpu_pair']})")
    assert_batch(res, "second_order2_1024", record_property)
    assert st["converged"].mean() >= 0.99 and it.mean() < 15.9          # fewer iterations than the default mode's 15.99
