"""Does the table of tests/consts_cases.py keep tests/test_gpu_consts.py honest?  No GPU, and nothing of the code under test: the numpy
oracle and the C oracle (oracle.cport, an independent statement) alone.
  (1) APPLIES is what the oracle says: moving a field alone changes f, F, g, H or L at the test points if and only if the (model,
      field) pair is listed -- and, for com and feet, component by component: what DevConsts drops (com x / y, the feet's z) is inert.
  (2) sensitive: every listed move changes the compared quantities by at least 1000 x the tolerance the GPU test compares them at, and
      so does the exchange of any two gain fields' values under ALL_OFF.
  (3) the two oracles agree at every case input within a tenth of that tolerance.
  (4) whole solves: the C oracle's two builds (-ffp-contract=off and fast) take the same number of iterations on every instance.
  (5) every sweep case passes the probe of tests/test_sweep_cases_cpu.py: a 1e-13 relative perturbation of the trajectory keeps the
      verdict and moves gains and rollouts by at most 1/100 of their tolerances.
A case that fails gets another value in the table, not another tolerance here."""
import numpy as np
import pytest

from oracle import cport, ddp as oddp
from tests import consts_cases as cc, oracle_refs as refs, sweep_cases as sc

PAIRS = [(m, f) for m in cc.MODELS for f in cc.FIELDS]
LISTED = [(m, f) for m, f in PAIRS if f in cc.APPLIES[m]]


def _base(model, field):
    """the constants a move of `field` is compared with: the defaults, with the friction barrier on where the field needs it"""
    return cc.moved(model, [], **(cc.FRICTION if field in cc.BAR else {}))


def _change(model, consts, base):
    return cc.knot_excess(cc.oracle_knots(model, consts), cc.oracle_knots(model, base))[0]


@pytest.mark.parametrize("model,field", PAIRS)
def test_applies_is_what_the_oracle_says_and_every_listed_move_shows(model, field):
    base = _base(model, field)
    ratio = _change(model, cc.moved(model, [field]), base)
    listed = field in cc.APPLIES[model]
    print(f"{model} {field}: the move changes f, F, H, g, L by {ratio:.3e} x the tolerance (listed: {listed})")
    if not listed:
        assert ratio == 0.0, (model, field, ratio)
        return
    assert ratio >= 1000.0, (model, field, ratio)
    if field in cc.COMPONENTS:      # the components DevConsts keeps carry the whole move; the others are inert to the bit
        read = cc.COMPONENTS[field].reshape(np.shape(base[field]))
        off = np.asarray(cc.off_value(model, field), dtype=float).reshape(read.shape)
        kept = _change(model, dict(base, **{field: np.where(read, off, base[field])}), base)
        dropped = _change(model, dict(base, **{field: np.where(read, base[field], off)}), base)
        print(f"{model} {field}: the components the kernels read alone {kept:.3e}, the others alone {dropped:.3e}")
        assert kept == ratio and dropped == 0.0, (model, field, kept, dropped)


@pytest.mark.parametrize("model", cc.MODELS)
def test_two_gains_exchanged_show(model):
    base = cc.ALL_OFF[model]
    ref = cc.oracle_knots(model, base)
    for i, a in enumerate(cc.GAINS):
        for b in cc.GAINS[i + 1:]:
            if a not in cc.APPLIES[model] and b not in cc.APPLIES[model]:
                continue
            ratio = cc.knot_excess(cc.oracle_knots(model, dict(base, **{a: base[b], b: base[a]})), ref)[0]
            print(f"{model}: {a} <-> {b} changes f, F, H, g, L by {ratio:.3e} x the tolerance")
            assert ratio >= 1000.0, (model, a, b, ratio)


def _cases(model):
    out = [(f, cc.moved(model, [f])) for f in cc.FIELDS if f in cc.APPLIES[model]]
    out += [("default", cc.defaults(model)), ("ALL_OFF", cc.ALL_OFF[model]), ("ALL_OFF bar", dict(cc.all_off(model, bar=True)))]
    return out + [(f"table[{b}]", row) for b, row in enumerate(cc.draw_all(model)[1])]


@pytest.mark.parametrize("model", cc.MODELS)
def test_the_two_oracles_agree_at_every_case_input(model):
    for name, consts in _cases(model):
        if model == "lip30" and consts.get("friction_barrier_weight", 0.0) > 0.0:
            continue                                       # lip30 has no forces: no barrier case
        worst, ex = cc.knot_excess(cc.oracle_knots(model, consts, numpy=False), cc.oracle_knots(model, consts))
        print(f"{model} {name}: numpy against C oracle {worst:.3e} of the tolerance ({', '.join(f'{k} {v:.1e}' for k, v in ex.items())})")
        assert worst <= 0.1, (model, name, ex)


@pytest.mark.parametrize("model", cc.MODELS)
def test_both_builds_of_the_c_oracle_take_the_same_iterations(model):
    N, seeds = cc.SOLVES[model]
    s = cc.problem(model, N, seeds)
    cst = cc.oracle_consts(model, s["consts"])
    st = {v: refs.c_oracle(model, s, cc.solve_options(model), v, cst=cst)[2] for v in ("off", "fast")}
    it, status = ({v: cport.stat(st[v], f).astype(int) for v in st} for f in ("iters", "status"))
    print(f"{model} N {N} seeds {seeds}: iterations off {it['off'].tolist()} fast {it['fast'].tolist()}; status {status['off'].tolist()}")
    np.testing.assert_array_equal(it["off"], it["fast"])
    np.testing.assert_array_equal(status["off"], status["fast"])
    assert (cport.stat(st["off"], "converged") == 1).all() and (it["off"] >= 1).all(), "a whole-solve case that does not converge, or has nothing to do"
    m = cc.oracle_model(model, s["consts"])      # and the numpy oracle, which the GPU test compares with, is on that count too
    opts = oddp.DdpOptions(**cc.solve_options(model))
    for b in range(len(seeds)):
        r = oddp.solve(m, s["x0"][b], s["params"][b], s["xs"][b], s["us"][b], opts)
        assert r.iters == it["off"][b] and r.converged, (model, b, r.iters)


@pytest.mark.parametrize("model,N,mode", [(m, N, 1) for m, N, _ in cc.SWEEPS] + [(m, N, 2) for m, N in cc.SO2_SWEEPS])
def test_sweep_cases_are_well_posed(model, N, mode):
    s, m, xs, us = cc.sweep_start(model, N, mode=mode)
    for b in range(len(xs)):
        ref, _, fw = cc.sweep_reference(m, s, xs, us, b, mode)
        assert ref.ok and all(np.isfinite(v[2]) for v in fw.values()), (model, b)
        rng = np.random.default_rng(b)
        xp = xs * (1.0 + sc.PROBE_A * rng.standard_normal(xs.shape))
        up = us * (1.0 + sc.PROBE_A * rng.standard_normal(us.shape))
        p, _, fwp = cc.sweep_reference(m, s, xp, up, b, mode)
        assert p.ok
        eK, ek = sc.gain_excess(p.K, ref.K), sc.gain_excess(p.kff, ref.kff)
        print(f"{model} N {N} [{b}]: a 1e-13 perturbation moves K by {eK:.2e}, kff by {ek:.2e} of the tolerance (allowed 1e-2)")
        assert eK <= 1e-2 and ek <= 1e-2, (model, b, eK, ek)
        for a, (xo, uo, Jo) in fw.items():
            xq, uq, Jq = fwp[a]
            ex, eu, eJ = np.max(np.abs(xq - xo)), np.max(np.abs(uq - uo)), abs(Jq - Jo) / abs(Jo)
            print(f"{model} N {N} [{b}]: rollout alpha {a:g} moves x by {ex:.2e}, u by {eu:.2e}, cost by {eJ:.2e} relative")
            assert ex <= 1e-10 and eu <= 1e-10 and eJ <= 1e-11 and np.max(np.abs(xo)) < 1e2, (model, b, a, ex, eu, eJ)
        # the constants matter to the sweep: the default robot's gains on the same trajectory differ by 1000 x the tolerance
        d, _, _ = cc.sweep_reference(cc.oracle_model(model, cc.defaults(model)), s, xs, us, b, mode)
        print(f"{model} N {N} [{b}]: ALL_OFF against the default robot changes K by {sc.spread(d.K, ref.K):.2e} (required 1e-4)")
        assert sc.spread(d.K, ref.K) >= 1000.0 * 1e-7, (model, b)
