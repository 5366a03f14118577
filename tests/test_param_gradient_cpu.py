"""Parameter sensitivities (include/sddp.h sddp_param_gradient_range_device), what needs no GPU: the symbolic reference of
tests/param_gradient_cases.py against tests/sym_models.py's own expressions and against central differences of the C oracle's f and L,
the parameter-name map of DDPSolver.parameter_gradient on a stub engine, and its refusals.

CENTRAL DIFFERENCES, one parameter entry at a time.  Every model's f is affine and its L a polynomial of degree 2 in any SINGLE entry
of p (rdot_ref, w_ref, c_ref, oref and, on srbd13, the contact points enter residual rows affinely; a switch and
orientation_tracking_gain multiply a row that does not read them): the third derivative along a coordinate is zero, a central
difference has NO truncation error at any step, and what is left is rounding.  With L0 = L(p), kappa = d2L/dp_j^2 (the second
difference at the trial step H0, exact for the same reason) and an evaluation error of E eps |L|,
    |difference quotient - dL/dp_j| <= E eps (L0 + kappa h^2 / 2) / h,      smallest at h = sqrt(2 L0 / kappa), where it is E eps sqrt(2 L0 kappa).
That h and that bound are the step and the tolerance, entry by entry; E = 64 is the project's margin for two correct float64 statements
of one sum of about a hundred terms (tests/stationarity_cases.py MARGIN).  An entry without curvature (kappa = 0: L does not read it,
or reads it affinely) keeps h = H0.  The reference's own rounding, E eps sum |2 r_i dr_i/dp_j|, is added.  For f the same holds with
kappa = 0: h = 1/4, tolerance E eps max |f| / h.
"""
import numpy as np
import pytest

from oracle import cport
from tests import param_gradient_cases as pg, sym_models as sm

EPS = np.finfo(np.float64).eps
E, H0 = 64.0, 1.0e-3


def _point(name, key, seed):
    """a random point (x, u, p) around the model's standing pose, the switches at 0 / 1"""
    _, x, u, P = pg.random_plan(name, 2, 1, seed)
    return x[0, 1], u[0, 1], P[0, 1]


@pytest.mark.parametrize("name", pg.MODELS)
def test_the_assembly_is_sym_models_own(name):
    """jacobians() on the default constants compiles the expressions of sym_models.symbolic(name)[0]["_sym"] (both are
    sym_models.assemble's): f and both residual vectors agree at random points to rounding"""
    xs, us, ps, f, ires, sres, _ = sm.symbolic(name)[0]["_sym"]
    import sympy as sp
    own = pg.jacobians(name)
    theirs = [sp.lambdify((list(xs), list(us), list(ps)), e, "numpy", cse=True) for e in (f, ires, sres)]
    for seed in (0, 1):
        x, u, p = _point(name, "default", seed)
        for mine, ref in zip((own["f"], own["ires"], own["sres"]), theirs):
            a, b = np.asarray(mine(x, u, p), dtype=float).reshape(-1), np.asarray(ref(x, u, p), dtype=float).reshape(-1)
            assert a.shape == b.shape and np.max(np.abs(a - b)) <= 8 * EPS * max(1.0, np.max(np.abs(b)))


@pytest.mark.parametrize("key", ("default", "off"))
@pytest.mark.parametrize("name", pg.MODELS)
def test_reference_against_central_differences_of_the_c_oracle(name, key):
    J, cst = pg.jacobians(name, key), pg.robot(name, key)
    N = 4
    worst = 0.0
    for seed, k in ((0, 0), (1, 2), (2, N)):                                   # node classes '0', 'k', 'N'
        x, u, p = _point(name, key, seed)
        terminal = k == N
        uu = np.zeros(J["nu"]) if terminal else u

        def both(q):
            f, _, _, _, L = cport.eval_knot(cst, x, uu, q, k, terminal, name)
            return np.array(f, dtype=float), L

        f0, L0 = both(p)
        assert abs(pg.cost(J, pg.node_class(k, N), x, None if terminal else u, p) - L0) <= E * EPS * max(1.0, abs(L0))
        g = pg.dL_dp(J, pg.node_class(k, N), x, None if terminal else u, p)
        Fp = np.broadcast_to(np.asarray(J["Fp"](x, u, p), dtype=float), (J["nx"], J["np"]))
        for j in range(J["np"]):
            e = np.zeros(J["np"]); e[j] = 1.0
            kappa = abs(both(p + H0 * e)[1] - 2.0 * L0 + both(p - H0 * e)[1]) / H0**2
            kappa = kappa if kappa * H0**2 > 1e3 * EPS * abs(L0) else 0.0      # a second difference below its own rounding is no curvature
            h = float(np.clip(np.sqrt(2.0 * L0 / kappa), 1e-6, 0.25)) if kappa > 0.0 and L0 > 0.0 else H0
            (fp, Lp), (fm, Lm) = both(p + h * e), both(p - h * e)
            own_rounding = E * EPS * (abs(g[j]) + 1.0)
            tol = E * EPS * (abs(L0) + 0.5 * kappa * h * h) / h + own_rounding
            err = abs((Lp - Lm) / (2.0 * h) - g[j])
            assert err <= tol, f"{name} {key} node {k} dL/dp[{j}]: {(Lp - Lm) / (2 * h)} against {g[j]}, tolerance {tol:.3e} at h = {h:.3e}"
            worst = max(worst, err / tol)
            if not terminal:
                hf = 0.25
                d = (both(p + hf * e)[0] - both(p - hf * e)[0]) / (2.0 * hf)
                tf = E * EPS * max(1.0, np.max(np.abs(f0))) / hf
                assert np.max(np.abs(d - Fp[:, j])) <= tf, f"{name} {key} node {k} df/dp[{j}]"
    print(f"{name} {key}: worst central-difference error / tolerance {worst:.3f}")
    if name != "srbd13":
        x, u, p = _point(name, key, 0)
        assert not np.any(np.asarray(J["Fp"](x, u, p), dtype=float))            # no parameter enters the dynamics
    else:
        assert sorted(set(np.nonzero(Fp)[1])) == list(range(11, 17)) and sorted(set(np.nonzero(Fp)[0])) == [10, 11, 12]


def test_node_gradient_adds_the_dynamics_term_in_order():
    J = pg.jacobians("srbd13")
    x, u, p = _point("srbd13", "default", 3)
    lam = np.random.default_rng(0).standard_normal(13)
    g, m = pg.node_gradient(J, 1, 4, x, u, p, lam)
    Fp = np.asarray(J["Fp"](x, u, p), dtype=float)
    assert np.allclose(g, pg.dL_dp(J, "k", x, u, p) + Fp.T @ lam, rtol=1e-13, atol=1e-9)
    assert np.all(m >= np.abs(g) - 1e-9)
    gN, _ = pg.node_gradient(J, 4, 4, x, None, p, None)
    assert np.array_equal(gN, pg.dL_dp(J, "N", x, None, p))


# ---- DDPSolver.parameter_gradient on a stub engine ----------------------------------------------------------------------------------------
class _StubEngine:
    """param_gradient of an engine: G[0, k, j] = 100 k + j, lambda_0 = 0 .. nx - 1"""
    def __init__(self, N, np_, nx):
        self.N, self.np_, self.nx, self.calls = N, np_, nx, 0

    def param_gradient(self, first, count, want_lambda=False):
        self.calls += 1
        assert (first, count, want_lambda) == (0, 1, True)
        G = (100.0 * np.arange(self.N + 1)[:, None] + np.arange(self.np_)[None, :])[None]
        rec = np.arange(8.0)[None]
        lam = np.zeros((1, self.N + 1, self.nx)); lam[0, 0] = np.arange(self.nx)
        return G, rec, lam

    def synchronize(self):
        pass


def _adapter(prb, np_model, nx, extra_refs=(), user=None):
    from srbd_horizon_amd.ddp import DDPSolver
    s = DDPSolver.__new__(DDPSolver)
    s.prb, s.param_var, s._np_model, s._extra_refs, s._user = prb, prb.getParameters(), np_model, list(extra_refs), user
    s.ddp_solver = _StubEngine(prb.nodes - 1, np_model + (8 if extra_refs else 0), nx)
    s.var_solution = {}
    return s


@pytest.mark.parametrize("maker,model", [(lambda: __import__("srbd_horizon_amd.prb", fromlist=["x"]).SRBDProblem().createSRBDProblem(6, 1.0), "srbd37"),
                                         (lambda: __import__("srbd_horizon_amd.prb", fromlist=["x"]).SRBD13Problem().createSRBD13Problem(6, 1.0), "srbd13"),
                                         (lambda: __import__("srbd_horizon_amd.prb", fromlist=["x"]).LIPProblem().createLIPProblem(6, 1.0), "lip30")])
def test_parameter_names_follow_the_parameter_matrix(maker, model):
    prb = maker()
    nx, _, np_ = sm.DIMS[model]
    s = _adapter(prb, np_, nx)
    out = s.parameter_gradient()
    # the columns of parameter_matrix(): every Parameter row by row in creation order.  Assigning column index j to every node of the
    # row that parameter_matrix() puts at column j must reproduce, in the dictionary, the stub's G[k, j] = 100 k + j
    col = 0
    for name, p in prb.getParameters().items():
        for r in range(p.getDim()):
            p.values[r, :] = col
            col += 1
    P = prb.parameter_matrix()
    assert P.shape == (prb.nodes, np_) and np.array_equal(P[0], np.arange(np_))
    assert set(out) == set(prb.getParameters()) | {"x0"}
    for name, p in prb.getParameters().items():
        assert out[name].shape == p.values.shape == (p.getDim(), prb.nodes)
        assert np.array_equal(out[name], p.values + 100.0 * np.arange(prb.nodes)[None, :]), name
    assert np.array_equal(out["x0"], np.arange(nx))
    assert s.parameter_gradient_record["gradient"] == 0.0 and s.parameter_gradient_record["nodes"] == 7.0
    expected = {"srbd37": {"rdot_ref", "w_ref", "orientation_tracking_gain", "oref", "c_ref0", "cdot_switch0", "c_ref3", "cdot_switch3"},
                "srbd13": {"rdot_ref", "w_ref", "orientation_tracking_gain", "oref", "c0", "c1", "cdot_switch0", "cdot_switch1"},
                "lip30": {"rdot_ref", "c_ref0", "cdot_switch0", "c_ref3", "cdot_switch3"}}[model]
    assert expected <= set(out)


def test_user_references_land_on_the_rows_that_read_them():
    from srbd_horizon_amd.prb import SRBD13Problem
    prb = SRBD13Problem().createSRBD13Problem(6, 1.0)
    ref = prb.createParameter("height_ref", 2)
    s = _adapter(prb, 19, 13, extra_refs=[(ref, 1), None, (ref, 0)])
    out = s.parameter_gradient()
    k = 100.0 * np.arange(prb.nodes)
    assert np.array_equal(out["height_ref"], np.stack([k + 19 + 2, k + 19 + 0]))
    assert np.array_equal(out["rdot_ref"], np.stack([k + 0, k + 1, k + 2]))


def test_refusals_on_a_stub():
    from srbd_horizon_amd.prb import SRBD13Problem
    prb = SRBD13Problem().createSRBD13Problem(6, 1.0)
    s = _adapter(prb, 19, 13)
    s.var_solution = None
    with pytest.raises(RuntimeError, match="no solve has run"):
        s.parameter_gradient()
    s = _adapter(prb, 19, 13, user=object())
    with pytest.raises(NotImplementedError, match="non-linear residuals"):
        s.parameter_gradient()
    assert s.ddp_solver.calls == 0


def test_envelope_experiment_on_the_c_oracle():
    """The envelope experiment of param_gradient_cases (srbd13, N = 8, four robots, a direction over rdot_ref and the footholds) with the C
    oracle's solves and the symbolic reference: all three solves of all four robots converge with closed gaps at every step (asserted
    inside), the figure falls as h^2 while truncation leads, and its smallest value over the scan and the h it is found at are the
    recorded ENVELOPE_DISCREPANCY and ENVELOPE_H (a rounding-level floor: to a factor of 2 on another CPU)."""
    scan = {h: d.max() for h, d in pg.envelope_scan().items()}
    for h, d in scan.items():
        print(f"h = {h:.0e}: discrepancy {d:.3e}")
    assert all(np.isfinite(d) for d in scan.values()) and len(scan) == len(pg.ENVELOPE_STEPS)
    assert 50.0 < scan[1e-2] / scan[1e-3] < 200.0                               # second order in h: G is the derivative, not near it
    best = min(scan, key=scan.get)
    assert 0.5 * pg.ENVELOPE_DISCREPANCY <= scan[best] <= 2.0 * pg.ENVELOPE_DISCREPANCY
    assert scan[pg.ENVELOPE_H] <= 2.0 * pg.ENVELOPE_DISCREPANCY and scan[pg.ENVELOPE_H] <= 1.1 * scan[best]
