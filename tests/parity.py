"""The two comparisons of a whole GPU solve with an oracle's, each written once, and the tolerances they hold -- numpy and pytest
only (tests/options_cases.py, which holds RHO_RTOL beside the figure it is derived from, needs no GPU either): CPU tests import this
module, tests/test_parity_helper_cpu.py pins every bound below.

Against the C oracle (cport.solve_batch: stats [B, 8] = cport.STAT_FIELDS): iters, status, converged and alpha exact (alpha:
the same double); mu rel 1e-12 (regularisation bump: exact factors of ten); l-inf of x and of u 1e-6 and cost rel 1e-9 (a converged
solve, fp64 on both sides); gap rel 1e-9 (the start's defect norm times exact factors 1 - alpha); rho within RHO_RTOL, ten times the
spread of the oracle's own two builds.
Against the numpy oracle's result object (oddp.solve), per instance: the same iteration count, l-inf 1e-6, cost rel 1e-9, gaps closed
to 1e-9.
A failed instance (status 2, 3, 4; assert_failed_matches_c_oracle): the same exact fields and the same bounds, no new one; cost and gap
non-finite exactly where the oracle's are; the trajectory either the start's bytes or the oracle's iterate at 1e-6 on its finite entries.
deviations() divides by the cost: failed instances go through failed_deviations(), which looks at the oracle's finite entries only."""
import numpy as np
import pytest

from oracle.cport import stat
from tests.options_cases import RHO_RTOL

X_TOL = 1e-6             # l-inf of x and of u
COST_RTOL = 1e-9
GAP_RTOL = 1e-9
MU_RTOL = 1e-12         # through pytest.approx(rel=...), whose absolute floor of 1e-12 holds beside it
GAP_CLOSED = 1e-9        # numpy oracle: a converged multiple-shooting solve has closed its gaps


def deviations(x, u, st, xo, uo, so):
    """-> dict(x, u: l-inf; cost, rho, gap: largest relative difference) over the batch"""
    rel = lambda f: float(np.max(np.abs(st[f] - stat(so, f)) / np.maximum(np.abs(stat(so, f)), 1e-300)))
    return dict(x=float(np.max(np.abs(x - xo))), u=float(np.max(np.abs(u - uo))),
                cost=float(np.max(np.abs(st["cost"] - stat(so, "cost")) / np.abs(stat(so, "cost")))), rho=rel("rho"), gap=rel("gap"))


def summary(d):
    return f"linf x {d['x']:.2e} u {d['u']:.2e}; rel cost {d['cost']:.2e}; rel rho {d['rho']:.2e}; rel gap {d['gap']:.2e}"


def assert_matches_c_oracle(x, u, st, xo, uo, so, *, gap_slack=0.0, explain=None):
    """x, u, st (sddp_stats records): the GPU's solve; xo, uo, so: cport.solve_batch's.  explain(differ) -> the failure text for the
    instances `differ` on another iteration count than the oracle (asked before anything else is asserted); gap_slack: absolute slack
    of the gap comparison, a number or one per instance."""
    B = len(st)
    it_o = stat(so, "iters").astype(int)
    differ = np.flatnonzero(st["iters"] != it_o)
    if differ.size and explain is not None:
        pytest.fail(explain(differ))
    np.testing.assert_array_equal(st["iters"], it_o)
    np.testing.assert_array_equal(st["status"], stat(so, "status").astype(int))
    np.testing.assert_array_equal(st["converged"], stat(so, "converged").astype(int))
    np.testing.assert_array_equal(st["alpha"], stat(so, "alpha"))                           # the same double
    slack = np.broadcast_to(gap_slack, (B,))
    cost, gap, mu, rho = (stat(so, f) for f in ("cost", "gap", "mu", "rho"))
    for b in range(B):
        assert st["mu"][b] == pytest.approx(mu[b], rel=MU_RTOL), (b, st["mu"][b], mu[b])
        ex, eu = np.max(np.abs(x[b] - xo[b])), np.max(np.abs(u[b] - uo[b]))
        assert ex <= X_TOL and eu <= X_TOL, (b, ex, eu)
        assert abs(st["cost"][b] - cost[b]) <= COST_RTOL * abs(cost[b]), (b, st["cost"][b], cost[b])
        assert abs(st["gap"][b] - gap[b]) <= GAP_RTOL * abs(gap[b]) + slack[b], (b, st["gap"][b], gap[b])
        assert abs(st["rho"][b] - rho[b]) <= RHO_RTOL * abs(rho[b]), (b, st["rho"][b], rho[b])


def assert_matches_numpy_oracle(x, u, st, r, b=None):
    """one instance: x [N+1, nx], u [N, nu] and its sddp_stats record st against the result r of oddp.solve; b: its label in messages"""
    assert st["iters"] == r.iters, (b, st["iters"], r.iters)
    ex, eu = np.max(np.abs(x - r.xs)), np.max(np.abs(u - r.us))
    assert ex <= X_TOL and eu <= X_TOL, (b, ex, eu)
    assert abs(st["cost"] - r.cost) <= COST_RTOL * abs(r.cost), (b, st["cost"], r.cost)
    assert st["gap"] <= GAP_CLOSED, (b, st["gap"])


def _close_or_same_non_finite(got, ref, rtol, what):
    """non-finite exactly where the oracle is (inf for inf of the same sign, NaN for NaN); within rtol where it is finite"""
    if np.isfinite(ref):
        assert np.isfinite(got) and abs(got - ref) <= rtol * abs(ref), (what, got, ref)
    elif np.isnan(ref):
        assert np.isnan(got), (what, got, ref)
    else:
        assert got == ref, (what, got, ref)


def failed_deviations(x, u, st, xo, uo, so, sel):
    """deviations() over the instances `sel`, on the finite entries of the oracle only (a failed instance may hold NaNs)"""
    sel = np.asarray(sel, dtype=int)
    def linf(a, b):
        m = np.isfinite(b)
        return float(np.max(np.abs(a[m] - b[m]))) if m.any() else 0.0
    def rel(f):
        g, o = st[f][sel], stat(so, f)[sel]
        m = np.isfinite(o) & (o != 0.0)
        return float(np.max(np.abs(g[m] - o[m]) / np.abs(o[m]))) if m.any() else 0.0
    return dict(x=linf(x[sel], xo[sel]), u=linf(u[sel], uo[sel]), cost=rel("cost"), gap=rel("gap"), rho=rel("rho"))


def assert_failed_matches_c_oracle(x, u, st, xo, uo, so, b, *, start=None, rollouts=None):
    """instance b of a GPU solve that gave up (status 2, 3 or 4) against cport.solve_batch's: status, iters, converged and alpha exact
    (alpha: the same double); mu rel MU_RTOL; cost and gap at COST_RTOL / GAP_RTOL where the oracle's are finite, non-finite exactly
    where they are not; rollouts exact where given.  The returned trajectory: start = (x0, xs, us) -> the start's bytes with row 0 =
    x0 (a solve that gave up before any accepted step on multiple shooting); None -> the oracle's iterate, the same non-finite mask
    and X_TOL on the finite entries."""
    assert st["status"][b] == int(stat(so, "status")[b]) and st["status"][b] in (2, 3, 4), (b, st["status"][b], stat(so, "status")[b])
    assert st["iters"][b] == int(stat(so, "iters")[b]), (b, st["iters"][b], stat(so, "iters")[b])
    assert st["converged"][b] == int(stat(so, "converged")[b]) == 0, (b, st["converged"][b])
    assert st["alpha"][b].tobytes() == np.float64(stat(so, "alpha")[b]).tobytes(), (b, st["alpha"][b], stat(so, "alpha")[b])
    if rollouts is not None:
        assert st["rollouts"][b] == rollouts, (b, st["rollouts"][b], rollouts)
    mu = stat(so, "mu")[b]
    assert st["mu"][b] == pytest.approx(mu, rel=MU_RTOL), (b, st["mu"][b], mu)
    _close_or_same_non_finite(st["cost"][b], stat(so, "cost")[b], COST_RTOL, ("cost", b))
    _close_or_same_non_finite(st["gap"][b], stat(so, "gap")[b], GAP_RTOL, ("gap", b))
    if start is not None:
        x0, xs, us = start
        want = np.array(xs, copy=True)
        want[0] = x0
        assert x[b].tobytes() == want.tobytes(), f"instance {b}: xs is not the start with row 0 = x0"
        assert u[b].tobytes() == np.ascontiguousarray(us).tobytes(), f"instance {b}: us is not the start"
        return
    for got, ref, what in ((x[b], xo[b], "x"), (u[b], uo[b], "u")):
        fin = np.isfinite(ref)
        np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=f"instance {b}: non-finite entries of {what}")
        e = float(np.max(np.abs(got[fin] - ref[fin]))) if fin.any() else 0.0
        assert e <= X_TOL, (b, what, e)
