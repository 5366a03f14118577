"""Does every row of tests/whole_solve_cases.py support the comparison the GPU tests make with it (parity.assert_matches_c_oracle:
iters, status, converged and alpha exact)?  The C oracle's two builds alone, no GPU: a row on which they disagree is no reference."""
import numpy as np
import pytest

from oracle import cport
from tests import options_cases as oc, parity, whole_solve_cases as wc


@pytest.mark.parametrize("name", list(wc.CASES))
def test_both_builds_of_the_c_oracle_agree_on_the_case(name):
    (xo, uo, so), (xf, uf, sf) = wc.oracle(name, "off"), wc.oracle(name, "fast")
    it = cport.stat(so, "iters").astype(int)
    rho, rho_f = cport.stat(so, "rho"), cport.stat(sf, "rho")
    linf = float(np.max(np.abs(xo - xf)))
    print(f"{name}: iterations {it.min()}-{it.max()}; builds differ in x by {linf:.2e}; rho max {rho.max():.3e}, gap max {cport.stat(so, 'gap').max():.3e}")
    for f in ("iters", "status", "converged", "alpha"):
        np.testing.assert_array_equal(cport.stat(so, f), cport.stat(sf, f), err_msg=f)
    assert (cport.stat(so, "status") == 0).all() and (cport.stat(sf, "status") == 0).all()
    assert (np.abs(rho - rho_f) <= oc.RHO_SPREAD * np.abs(rho)).all(), (rho, rho_f)
    assert linf <= 0.1 * parity.X_TOL, linf
    assert (it.min(), it.max()) == wc.ITERS[name]
