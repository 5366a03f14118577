"""Does the table of tests/sweep_cases.py keep tests/test_gpu_sweep_modes.py honest?  No GPU, and nothing of the code under test: the
numpy oracle alone.  For every case
  (a) well-conditioned: the oracle's sweep from a copy of the trajectory perturbed by 1e-13 relative moves K and kff by at most 1/100
      of the tolerance the GPU test compares them at, and the rollouts with those gains by at most 1/100 of theirs -- a kernel that
      differs from the oracle by rounding passes with room;
  (b) discriminating: the oracle's gains without the term the case is there for differ by at least 1000 x that tolerance --
      theta = 0 instead of 1 (SRBD models), the second_order = 1 term instead of the full tensor (second_order = 2 builds), the true
      defects instead of d = 0 (closed cases, in kff) -- so a kernel that dropped or mangled the term cannot pass.
lip30 is linear-quadratic: there theta must change nothing, to the bit.  A rejection case has to keep its verdict on 8 copies of the
iterate perturbed by 1e-10 relative.  A case that fails is replaced in the table, not exempted here."""
import numpy as np
import pytest

from oracle import ddp as oddp
from tests import sweep_cases as sc

ALL = [c.name for c in sc.cases()]
FACTOR_B = 1000.0 * 1e-7      # 1000 x the relative tolerance of the gains, as a change relative to max(1, max|gain|)


@pytest.mark.parametrize("name", [n for n in ALL if not sc.CASES[n].reject])
def test_case_is_well_conditioned_and_discriminating(name):
    case = sc.CASES[name]
    for b in range(len(case.seeds)):
        ref = sc.reference(name)[b][0]
        assert ref.ok, (name, b, "the oracle rejects the case's own sweep")
        assert all(np.isfinite(v[2]) for v in sc.reference(name)[b][2].values()), (name, b, "a rollout of the case is not finite")
        # (a)
        xp, up = sc.perturbed(case, b, sc.PROBE_A, seed=b)
        p = sc.sweep(case, b, xp, up)
        assert p.ok
        eK, ek = sc.gain_excess(p.K, ref.K), sc.gain_excess(p.kff, ref.kff)
        print(f"{name}[{b}] (a): a 1e-13 perturbation moves K by {eK:.2e}, kff by {ek:.2e} of the tolerance (allowed 1e-2); "
              f"K by {sc.spread(p.K, ref.K):.2e} of max(1, max|K|)")
        assert eK <= 1e-2 and ek <= 1e-2, (name, b, eK, ek)
        # ... and the rollouts with those gains by at most 1/100 of theirs (x, u 1e-8; cost 1e-9 relative)
        s = sc.start(case)
        m, P = s["models"][b], s["params"][b]
        dp = oddp.defects(m, xp, up, P) if case.gaps == "open" else np.zeros((case.N, m.nx))
        for a, (xo, uo, Jo) in sc.reference(name)[b][2].items():
            xq, uq, Jq = oddp.forward_pass(m, s["x0"][b], xp, up, P, dp, p.K, p.kff, a)
            ex, eu, eJ = np.max(np.abs(xq - xo)), np.max(np.abs(uq - uo)), abs(Jq - Jo) / abs(Jo)
            print(f"{name}[{b}] (a): rollout alpha {a:g} moves x by {ex:.2e}, u by {eu:.2e}, cost by {eJ:.2e} relative")
            assert ex <= 1e-10 and eu <= 1e-10 and eJ <= 1e-11 and np.max(np.abs(xo)) < 1e2, (name, b, a, ex, eu, eJ)
        # (b)
        if case.model == "lip30":
            other = sc.sweep(case, b, theta=1.0 - case.theta)
            assert other.ok and np.array_equal(other.K, ref.K) and np.array_equal(other.kff, ref.kff)
            continue
        if case.theta:
            g0 = sc.sweep(case, b, theta=0.0)
            print(f"{name}[{b}] (b): theta 1 against 0 changes K by {sc.spread(g0.K, ref.K):.2e} (required {FACTOR_B:.0e})")
            assert g0.ok and sc.spread(g0.K, ref.K) >= FACTOR_B, (name, b)
            if sc.mode_of(case) == 2:
                g1 = sc.sweep(case, b, mode=1)
                print(f"{name}[{b}] (b): mode 2 against mode 1 changes K by {sc.spread(g1.K, ref.K):.2e}")
                assert g1.ok and sc.spread(g1.K, ref.K) >= FACTOR_B, (name, b)
        if case.gaps == "closed":
            gd = sc.sweep(case, b, gaps="open")
            print(f"{name}[{b}] (b): the true defects against d = 0 change kff by {sc.spread(gd.kff, ref.kff):.2e}")
            assert gd.ok and sc.spread(gd.kff, ref.kff) >= FACTOR_B, (name, b)


@pytest.mark.parametrize("name", [n for n in ALL if sc.CASES[n].reject])
def test_rejection_verdict_is_robust(name):
    case = sc.CASES[name]
    for b in range(len(case.seeds)):
        assert not sc.reference(name)[b][0].ok, (name, b, "the oracle accepts the sweep")
        assert sc.sweep(case, b, theta=0.0).ok, (name, b, "rejected without the second-order term as well: not the fallback's case")
        for seed in range(8):
            xp, up = sc.perturbed(case, b, sc.PROBE_REJECT, seed=seed)
            assert not sc.sweep(case, b, xp, up).ok, (name, b, seed)


def test_the_table_holds_the_matrix():
    """every row of the matrix: model x build x horizons, and both kernel families' poison cases exist"""
    have = {(c.model, c.build, c.N, c.gaps) for c in sc.cases() if not c.reject}
    for N in (1, 3, 65):
        for g in ("open", "closed"):
            assert ("srbd13", "plain", N, g) in have
            assert {(c.theta, c.mu) for c in sc.cases() if (c.model, c.build, c.N, c.gaps) == ("srbd13", "plain", N, g)} == \
                {(t, m) for t in (0.0, 1.0) for m in (0.0, 1e-6, 1e-2)}
    for N in (1, 3, 30):
        assert ("srbd13", "so2", N, "open") in have and ("srbd13", "so2", N, "closed") in have
    for bld in ("so2-conv", "so2-friction", "friction", "bound", "table"):
        assert ("srbd13", bld, 3, "closed") in have
    assert ("srbd13", "x", 3, "open") in have and ("srbd37", "so2-friction", 2, "open") in have
    for bld in ("plain", "so2"):
        for N in (2, 20):
            assert {(c.theta, c.mu) for c in sc.cases() if (c.model, c.build, c.N) == ("srbd37", bld, N) and not c.reject} == \
                {(t, m) for t in (0.0, 1.0) for m in (0.0, 1e-6)}
    assert {c.N for c in sc.cases() if c.model == "srbd61"} == {1, 6} and {c.N for c in sc.cases() if c.model == "lip30"} == {2, 20}
    assert sum(c.reject for c in sc.cases()) == 2
    assert all(n in sc.CASES for n in sc.POISON_CASES)
    assert len(ALL) == len(set(ALL))
