"""The table of tests/failure_build_cases.py on the oracles, no GPU: every case of every build with traits ends the way the table says on
both builds of the C oracle (the user build: on its one reference, the numpy oracle with the user rows), the builds agree on iters,
status, converged and alpha to the bit on every instance of the mixed batch and of its all-healthy twin, every failing cost is
non-finite or below 1e290, every healthy instance ends with status 0, the build-specific faults fail for the reason the table gives
(S3v, S3f: finite without the barrier; S3x: finite without the one inf), the mid-solve cases (S4b) and the healthy solves with a
rejected overflowed rung (Lc) agree between the numpy and the C oracle within the bounds of tests/parity.py.  Each test prints the
oracle's status per instance and, for Lc, the rungs rejected for a non-finite cost."""
import numpy as np
import pytest

from oracle import cport, ddp as oddp, models as omodels
from tests import failure_build_cases as fb, parity

NAMES = list(fb.CASES)
C_ORACLE = [n for n in NAMES if fb.CASES[n].build != "user"]
FINITE_BELOW = 1e290                                                   # the kernels test |J| < 1e300, the oracle isfinite


def _same_decisions(a, b):
    for f in ("iters", "status", "converged"):
        np.testing.assert_array_equal(cport.stat(a, f), cport.stat(b, f), err_msg=f)
    assert cport.stat(a, "alpha").tobytes() == cport.stat(b, "alpha").tobytes()


def test_the_table_covers_every_build_with_traits():
    from srbd_horizon_amd import _lib
    trait_builds = {(b.model, frozenset(b.traits)) for b in _lib.INSTANCES if b.traits}
    traits = {"x": {"xr"}, "friction": {"bar"}, "bound": {"bar"}, "so2": {"so2"}, "so2-friction": {"bar", "so2"}}
    covered = {(m, frozenset(traits[b])) for b, models in fb.BUILDS.items() if b != "user" for m in models}
    assert covered == trait_builds
    assert fb.SHAPES is fb.fc.SHAPES and fb.FAIL is fb.fc.FAIL
    for c in fb.CASES.values():
        assert len(c.seeds) == fb.SHAPES[c.model][1] and c.N == fb.SHAPES[c.model][0]


@pytest.mark.parametrize("name", fb.FAILING)
def test_case_ends_the_way_the_table_says_on_both_builds(name):
    c = fb.CASES[name]
    want, fail = fb.expected_status(c), list(c.fail)
    for variant in fb.variants(c):
        st = fb.oracle(name, variant)[2]
        print(f"{name} [{variant}]: status {cport.stat(st, 'status').astype(int).tolist()} iters {cport.stat(st, 'iters').astype(int).tolist()}")
        np.testing.assert_array_equal(cport.stat(st, "status"), want)
        np.testing.assert_array_equal(cport.stat(st, "converged"), (want == 0).astype(float))
        assert (cport.stat(st, "alpha")[fail] == 0.0).all()
        if c.kind == "S4b":
            np.testing.assert_array_equal(cport.stat(st, "iters")[fail], fb.MID_ITERS[name])
        else:
            assert (cport.stat(st, "iters")[fail] == 0).all()
        cost = cport.stat(st, "cost")[fail]
        if c.kind.startswith("S3"):
            assert not np.isfinite(cost).any() and (cport.stat(st, "mu")[fail] == 0.0).all()
        else:
            assert (np.abs(cost) < FINITE_BELOW).all()
    if len(fb.variants(c)) == 2:
        _same_decisions(fb.oracle(name, "off")[2], fb.oracle(name, "fast")[2])


@pytest.mark.parametrize("name", fb.MIXED)
def test_healthy_instances_are_their_solves_in_the_all_healthy_batch(name):
    c = fb.CASES[name]
    h = fb.healthy_idx(c)
    assert len(h) and len(h) + len(c.fail) == len(c.seeds)
    s, t = fb.start(name), fb.healthy(name)
    for k in ("x0", "params", "xs", "us"):
        assert s[k][h].tobytes() == t[k][h].tobytes(), k
    for variant in fb.variants(c):
        mixed, twin = fb.oracle(name, variant), fb.oracle(name, variant, True)
        assert (cport.stat(twin[2], "status") == 0).all() and (cport.stat(twin[2], "converged") == 1).all()
        for a, b in zip(mixed, twin):
            assert a[h].tobytes() == b[h].tobytes()
    if len(fb.variants(c)) == 2:
        _same_decisions(fb.oracle(name, "off", True)[2], fb.oracle(name, "fast", True)[2])


@pytest.mark.parametrize("name", [n for n in NAMES if fb.CASES[n].kind == "S2"])
def test_status_2_ends_after_one_bump_with_the_start_returned(name):
    c, s = fb.CASES[name], fb.start(name)
    opt = oddp.DdpOptions(**fb.options(c))
    for variant in fb.variants(c):
        xs, us, st = fb.oracle(name, variant)
        assert (cport.stat(st, "mu") == 10.0 * fb.fc.MU0_S2 + opt.mu_min).all()
        want = s["xs"].copy()
        want[:, 0] = s["x0"]
        assert xs.tobytes() == want.tobytes() and us.tobytes() == s["us"].tobytes()
        assert np.isfinite(cport.stat(st, "cost")).all()


@pytest.mark.parametrize("name", [n for n in NAMES if fb.CASES[n].kind in ("S3x", "S3v", "S3f")])
def test_the_build_specific_fault_is_the_only_reason_for_status_3(name):
    """S3x: every base column finite, one widened column inf, and the plain model's cost of the same start finite.  S3v, S3f: a finite
    input; the start cost is +inf with the barrier and finite, far below 1e290, with its weight set to 0"""
    c, s = fb.CASES[name], fb.start(name)
    f, npb = list(c.fail), fb.base_columns(c.model)
    assert np.isfinite(s["params"][:, :, :npb]).all()
    if c.kind == "S3x":
        bad = ~np.isfinite(s["params"])
        assert bad.sum() == len(f) and bad[f, c.N // 2, npb].all() and np.isposinf(s["params"][f, c.N // 2, npb]).all()
        plain = dict(s, params=np.ascontiguousarray(s["params"][:, :, :npb]), consts=s["base_consts"])
        cost = cport.stat(fb.refs.c_oracle(c.model, plain, fb.options(c, max_iters=0))[2], "cost")
        assert (np.abs(cost) < FINITE_BELOW).all()
        assert not np.isfinite(fb.start_cost(name)[f]).any()
        return
    assert all(np.isfinite(s[k]).all() for k in ("x0", "xs", "us", "params"))
    weight = "bound_barrier_weight" if c.kind == "S3v" else "friction_barrier_weight"
    for variant in fb.variants(c):
        with_barrier, without = fb.start_cost(name, variant), fb.start_cost(name, variant, **{weight: 0.0})
        print(f"{name} [{variant}]: start cost {with_barrier.tolist()}; with {weight} = 0: {without.tolist()}")
        assert np.isposinf(with_barrier[f]).all() and np.isfinite(with_barrier[fb.healthy_idx(c)]).all()
        assert (np.abs(without) < FINITE_BELOW).all()
    if c.kind == "S3f":
        A = omodels.friction_cone_rows(s["consts"].get("friction_cone_coefficient", omodels.RobotConsts().friction_cone_coefficient))
        for b in f:
            k, (fz, sw) = fb.stance_knot(c.model, s["params"][b]), fb._fz(c.model)
            assert s["params"][b, k, sw] == 1.0
            arg = s["consts"]["friction_barrier_sharpness"] * (A @ s["us"][b, k, fz - 2:fz + 1])
            assert (arg >= fb.CONE_ARGUMENT).sum() == 1, arg


def _numpy_agrees(c, s, m, xo, uo, so, b):
    with np.errstate(all="ignore"):
        r = oddp.solve(m, s["x0"][b], s["params"][b], s["xs"][b], s["us"][b], oddp.DdpOptions(**fb.options(c)))
    assert (r.status, r.iters, int(r.converged)) == tuple(int(cport.stat(so, f)[b]) for f in ("status", "iters", "converged")), b
    assert r.alpha == cport.stat(so, "alpha")[b] and r.mu == pytest.approx(cport.stat(so, "mu")[b], rel=parity.MU_RTOL)
    cost = cport.stat(so, "cost")[b]
    if np.isfinite(cost):
        assert abs(r.cost - cost) <= parity.COST_RTOL * abs(cost), (b, r.cost, cost)
        assert np.max(np.abs(r.xs - xo[b])) <= parity.X_TOL and np.max(np.abs(r.us - uo[b])) <= parity.X_TOL, b
    else:
        assert not np.isfinite(r.cost)


NUMPY = [n for n in C_ORACLE if fb.CASES[n].kind in ("S4b", "Lc", "S3v", "S3f") or (fb.CASES[n].kind in ("S2", "S40") and fb.CASES[n].model == "srbd13")]


@pytest.mark.parametrize("name", NUMPY)
def test_numpy_oracle_agrees_with_the_c_oracle(name):
    """every failing instance of a mid-solve case and every instance of an Lc case (the table's criterion for a seed); one failing
    instance of the others"""
    c, s = fb.CASES[name], fb.start(name)
    m = omodels.make_model(c.model, fb.refs.consts(s))
    xo, uo, so = fb.oracle(name)
    which = c.fail if c.kind == "S4b" else range(len(c.seeds)) if c.kind == "Lc" else c.fail[1:2]
    for b in which:
        _numpy_agrees(c, s, m, xo, uo, so, b)


@pytest.mark.parametrize("name", list(fb.LC))
def test_a_healthy_solve_rejects_an_overflowed_rung(name):
    """Lc: status 0 and converged on every instance, on both builds with the same decisions; every instance's trace holds a line search
    with a non-finite margin on a rung in front of the accepted one, the same rungs on both builds; every finite candidate cost of
    the trace is below 1e290"""
    c = fb.CASES[name]
    a, b = fb.oracle(name, "off")[2], fb.oracle(name, "fast")[2]
    _same_decisions(a, b)
    assert (cport.stat(a, "status") == 0).all() and (cport.stat(a, "converged") == 1).all()
    for i in range(len(c.seeds)):
        tr = fb.oracle_trace(name, i)
        rungs = fb.rejected_non_finite(tr)
        print(f"{name} instance {i} (seed {c.seeds[i]}): {len(tr)} line searches, {int(cport.stat(a, 'iters')[i])} iterations, "
              f"rejected non-finite rungs (search, rung) {rungs}; rollouts {fb.expected_rollouts(c.model, tr)}")
        assert rungs and rungs == fb.rejected_non_finite(fb.oracle_trace(name, i, "fast"))
        assert fb.expected_rollouts(c.model, tr) == fb.expected_rollouts(c.model, fb.oracle_trace(name, i, "fast"))
        for r in tr:
            J = np.concatenate([r["J_cand"], [r["J"]]])
            assert (np.abs(J[np.isfinite(J)]) < FINITE_BELOW).all()

