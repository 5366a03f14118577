"""The two comparisons of a whole GPU solve with an oracle's, each written once, and the tolerances they hold -- numpy and pytest
only (tests/options_cases.py, which holds RHO_RTOL beside the figure it is derived from, needs no GPU either): CPU tests import this
module, tests/test_parity_helper_cpu.py pins every bound below.

Against the C oracle (cport.solve_batch: stats [B, 8] = options_cases.STAT_FIELDS): iters, status, converged and alpha exact (alpha:
the same double); mu rel 1e-12 (regularisation bump: exact factors of ten); l-inf of x and of u 1e-6 and cost rel 1e-9 (a converged
solve, fp64 on both sides); gap rel 1e-9 (the start's defect norm times exact factors 1 - alpha); rho within RHO_RTOL, ten times the
spread of the oracle's own two builds.
Against the numpy oracle's result object (oddp.solve), per instance: the same iteration count, l-inf 1e-6, cost rel 1e-9, gaps closed
to 1e-9."""
import numpy as np
import pytest

from tests.options_cases import RHO_RTOL, stat

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
