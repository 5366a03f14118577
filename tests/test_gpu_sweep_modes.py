"""The sweep's second-order and closed-gap paths, and the regularised sweep, against the numpy oracle: one backward sweep and three
rollouts per case of tests/sweep_cases.py (B = 2), through DdpEngine.backward(params, mu, theta, closed) / forward(params, alpha,
closed).  In a solve these paths run in every iteration after the first full step, where a wrong term changes the path and not the
optimum; here a wrong entry of v'.f_ux, of the v'.f_zz tensor or of the closed-gap branch misses the gains by three orders or more
(tests/test_sweep_cases_cpu.py, condition b).  Tolerances: sweep_cases' module docstring -- the project's for one sweep, no case has
its own.  What this does not reach: the non-linear rows of the user builds (tests/test_gpu_user_terms.py)."""
import numpy as np
import pytest

from tests import sweep_cases as sc

pytestmark = pytest.mark.gpu


def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", [c.name for c in sc.cases()])
def test_sweep_and_rollouts_match_the_oracle(name):
    case, s = sc.CASES[name], sc.start(sc.CASES[name])
    P, closed = s["params"], case.gaps == "closed"
    ref = sc.reference(name)
    eng = sc.make_engine(case)
    kff, K, scal = eng.backward(P, case.mu, case.theta, closed)
    kff, K, scal = kff.copy(), K.copy(), scal.copy()
    if case.reject:          # the verdict that sends a solve back to theta = 0; nothing else is defined after a rejected sweep
        for b in range(len(case.seeds)):
            print(f"{name}[{b}]: oracle ok {ref[b][0].ok}, engine ok {scal[b, 4]}")
            assert not ref[b][0].ok and scal[b, 4] == 0.0, (name, b, scal[b])
    else:
        assert (scal[:, 5] == case.mu).all()
        for b in range(len(case.seeds)):
            sc.assert_sweep_matches(kff[b], K[b], scal[b], ref[b], f"{name}[{b}]")
        for alpha in sc.ALPHAS:
            x, u, J = eng.forward(P, alpha, closed)
            for b in range(len(case.seeds)):
                sc.assert_rollout_matches(x[b], u[b], J[b], ref[b], alpha, f"{name}[{b}]")
        if case.model == "lip30":      # linear-quadratic: there is no second-order term, theta must not change a bit
            k0, K0, s0 = eng.backward(P, case.mu, 1.0 - case.theta, closed)
            np.testing.assert_array_equal(k0, kff)
            np.testing.assert_array_equal(K0, K)
            np.testing.assert_array_equal(s0, scal)
    # the mode was this call's: a plain backward() afterwards is the one of a handle that never saw a mode
    after = eng.backward(P)
    fresh = sc.make_engine(case)
    _same(after, fresh.backward(P))
    _same(eng.forward(P, 0.25), fresh.forward(P, 0.25))
    eng.close(); fresh.close()


@pytest.mark.parametrize("name", ["srbd37-plain-N2-open-th1-mu1e-06", "lip30-plain-N2-open-th1-mu1e-06", "srbd61-plain-N1-open-th1-mu1e-06"])
def test_closed_gaps_are_refused_on_the_four_wavefront_kernels(name):
    case, P = sc.CASES[name], sc.start(sc.CASES[name])["params"]
    eng, fresh = sc.make_engine(case), sc.make_engine(case)
    ref = fresh.backward(P)
    with pytest.raises(RuntimeError, match="one-wavefront kernels only"):
        eng.backward(P, case.mu, case.theta, closed=True)
    with pytest.raises(RuntimeError, match="one-wavefront kernels only"):
        eng.forward(P, 0.25, closed=True)
    _same(eng.backward(P), ref)                    # a refused call leaves the default mode behind
    eng.close(); fresh.close()
