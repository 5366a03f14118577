"""The table of tests/failure_cases.py on the oracles, no GPU: every case ends with the status, iteration count and converged flag the
table records, on both builds of the C oracle; the builds agree on iters, status, converged and alpha to the bit on EVERY instance,
failing or healthy, of the mixed batch and of its all-healthy twin (so no instance of the table has to be left out of a GPU
comparison); a healthy instance of a mixed batch is its solve in the all-healthy batch; status 2 ends with mu = 10 * 2e300 + mu_min
exactly and the start returned; the numpy oracle agrees with the C oracle on S2 and on one S3 and one S4 case per model (this extends
the pin of tests/test_oracle_c.py to the failure exits and to the pivot's upper bound, which both oracles state since this table)."""
import numpy as np
import pytest

from oracle import cport, ddp as oddp, models as omodels
from tests import failure_cases as fc, parity

NAMES = list(fc.CASES)


def _same_decisions(a, b):
    for f in ("iters", "status", "converged"):
        np.testing.assert_array_equal(cport.stat(a, f), cport.stat(b, f), err_msg=f)
    assert cport.stat(a, "alpha").tobytes() == cport.stat(b, "alpha").tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_case_ends_the_way_the_table_says_on_both_builds(name):
    c = fc.CASES[name]
    want = fc.expected_status(c)
    fail = list(c.fail)
    for variant in ("off", "fast"):
        st = fc.oracle(name, variant)[2]
        np.testing.assert_array_equal(cport.stat(st, "status"), want)
        np.testing.assert_array_equal(cport.stat(st, "converged"), (want == 0).astype(float))
        assert (cport.stat(st, "alpha")[fail] == 0.0).all()
        if c.kind == "S4m":
            np.testing.assert_array_equal(cport.stat(st, "iters")[fail], fc.MID_ITERS[name])
        else:
            assert (cport.stat(st, "iters")[fail] == 0).all()
        cost = cport.stat(st, "cost")[fail]
        if c.kind.startswith("S3"):
            assert not np.isfinite(cost).any() and (cport.stat(st, "mu")[fail] == 0.0).all()
        else:
            assert (np.abs(cost) < 1e290).all()                          # the kernels test |J| < 1e300, the oracle isfinite
    _same_decisions(fc.oracle(name, "off")[2], fc.oracle(name, "fast")[2])


@pytest.mark.parametrize("name", fc.MIXED)
def test_healthy_instances_are_their_solves_in_the_all_healthy_batch(name):
    c = fc.CASES[name]
    h = fc.healthy_idx(c)
    assert len(h) and len(h) + len(c.fail) == len(c.seeds)
    assert 0 in c.fail and len(c.seeds) - 1 in c.fail and any(b + 1 in c.fail for b in c.fail)
    s, t = fc.start(name), fc.healthy(name)
    for k in ("x0", "params", "xs", "us"):
        assert s[k][h].tobytes() == t[k][h].tobytes(), k
    for variant in ("off", "fast"):
        mixed, twin = fc.oracle(name, variant), fc.oracle(name, variant, True)
        assert (cport.stat(twin[2], "status") == 0).all() and (cport.stat(twin[2], "converged") == 1).all()
        for a, b in zip(mixed, twin):
            assert a[h].tobytes() == b[h].tobytes()
    _same_decisions(fc.oracle(name, "off", True)[2], fc.oracle(name, "fast", True)[2])


@pytest.mark.parametrize("model", fc.MODELS)
def test_status_2_ends_after_one_bump_with_the_start_returned(model):
    name = f"S2-{model}"
    c, s = fc.CASES[name], fc.start(name)
    opt = oddp.DdpOptions(**fc.options(c))
    assert 10.0 * fc.MU0_S2 + opt.mu_min > opt.mu_max and np.isfinite(10.0 * fc.MU0_S2)
    for variant in ("off", "fast"):
        xs, us, st = fc.oracle(name, variant)
        assert (cport.stat(st, "mu") == 10.0 * fc.MU0_S2 + opt.mu_min).all()
        want = s["xs"].copy()
        want[:, 0] = s["x0"]
        assert xs.tobytes() == want.tobytes() and us.tobytes() == s["us"].tobytes()
    start_cost = cport.stat(fc.oracle(name)[2], "cost")
    assert np.isfinite(start_cost).all()


@pytest.mark.parametrize("name", [f"{k}-{m}" for m in fc.MODELS for k in ("S2", "S3b", "S40")] + list(fc.MID))
def test_numpy_oracle_agrees_with_the_c_oracle(name):
    c, s = fc.CASES[name], fc.start(name)
    m = omodels.make_model(c.model, fc.consts(name))
    xo, uo, so = fc.oracle(name)
    for b in (c.fail if name in fc.MID else c.fail[1:2]):                 # mid-solve: every failing instance (the table's criterion)
        _numpy_agrees(c, s, m, xo, uo, so, b)


def _numpy_agrees(c, s, m, xo, uo, so, b):
    with np.errstate(all="ignore"):
        r = oddp.solve(m, s["x0"][b], s["params"][b], s["xs"][b], s["us"][b], oddp.DdpOptions(**fc.options(c)))
    assert (r.status, r.iters, int(r.converged)) == tuple(int(cport.stat(so, f)[b]) for f in ("status", "iters", "converged"))
    assert r.alpha == cport.stat(so, "alpha")[b] and r.mu == pytest.approx(cport.stat(so, "mu")[b], rel=parity.MU_RTOL)
    cost = cport.stat(so, "cost")[b]
    if np.isfinite(cost):
        assert abs(r.cost - cost) <= parity.COST_RTOL * abs(cost)
        assert np.max(np.abs(r.xs - xo[b])) <= parity.X_TOL and np.max(np.abs(r.us - uo[b])) <= parity.X_TOL
    else:
        assert not np.isfinite(r.cost)


def test_the_pivot_bound_is_the_same_in_both_oracles():
    """a Quu pivot must lie in (0, 1e300): srbd13 at mu = 2e300 fails the sweep, at mu = 0.5e300 it passes (pivots ~5e299)"""
    name = "S2-srbd13"
    c, s = fc.CASES[name], fc.start(name)
    m = omodels.make_model(c.model, fc.consts(name))
    xs = s["xs"][0].copy(); xs[0] = s["x0"][0]
    d = oddp.defects(m, xs, s["us"][0], s["params"][0])
    assert oddp.PIVOT_MAX == 1e300
    assert not oddp.backward_pass(m, xs, s["us"][0], s["params"][0], d, fc.MU0_S2)[0]
    assert oddp.backward_pass(m, xs, s["us"][0], s["params"][0], d, 0.25 * fc.MU0_S2)[0]


@pytest.mark.parametrize("model", fc.MODELS)
def test_the_policy_rule_gives_no_policy_behind_status_2_and_3(model):
    """tests/policy_cases.py on the oracle's own failed records: behind S2 the sweep at mu = 2e301 fails and the bump passes mu_max;
    behind S3c no sweep is made (on srbd37, lip30 and srbd61 it would pass -- Quu does not depend on u -- and carry the NaN)"""
    from tests import policy_cases as pc
    m = omodels.make_model(model, fc.consts(f"S2-{model}"))
    for kind in ("S2", "S3c"):
        name = f"{kind}-{model}"
        c, s = fc.CASES[name], fc.start(name)
        opt = oddp.DdpOptions(**fc.options(c))
        xo, uo, so = fc.oracle(name)
        b = c.fail[0]
        stats = {f: cport.stat(so, f)[b] for f in cport.STAT_FIELDS}
        with np.errstate(all="ignore"):
            kff, K, info = pc.oracle_policy(m, xo[b], uo[b], s["params"][b], stats, opt, 3)
            if kind == "S3c":
                swept = oddp.backward_pass(m, xo[b], uo[b], s["params"][b], np.zeros((c.N, m.nx)), 0.0)
                # the sweep the rule refuses to make: it passes where Quu does not depend on u, and its dV1 is the NaN
                assert swept[0] == (model != "srbd13") and (model == "srbd13" or np.isnan(swept[3])), (name, swept[0], swept[3])
        mu = 10.0 * stats["mu"] + opt.mu_min if kind == "S2" else stats["mu"]
        assert info.tobytes() == np.array([mu, 0.0, 0.0, 0.0]).tobytes(), (name, info)
        assert not kff.any() and not K.any()
