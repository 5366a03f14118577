"""Can the table of tests/queue_order_cases.py tell a right queue order from a wrong one?  No GPU: the C oracle in its two builds
(`off`, `fast`; the numpy oracle for the user build) on every case.  The figures asserted here are the ones the module docstring of
tests/queue_order_cases.py states; an input that has drifted shows here first."""
import numpy as np
import pytest

from oracle import cport, ddp as oddp, models as omodels
from tests import queue_order_cases as qc

KEYS = list(qc.KEY_CASES)


def test_the_table_is_the_one_the_issue_asks_for():
    by_kind = {}
    for c in qc.KEY_CASES.values():
        by_kind.setdefault(c.kind, []).append((c.model, c.N, c.build))
    assert by_kind["plain"] == [("srbd13", 30, "plain")] * 2 + [("srbd37", 20, "plain"), ("lip30", 20, "plain"), ("srbd61", 12, "plain")]
    assert by_kind["horizon"] == [("srbd13", N, "plain") for N in (63, 64, 65, 129)] + [("srbd37", 65, "plain"), ("lip30", 64, "plain")]
    assert by_kind["builds"] == [("srbd13", 30, "x"), ("srbd37", 20, "x"), ("srbd13", 30, "friction"), ("srbd13", 30, "bound"),
                                 ("srbd13", 30, "so2"), ("srbd13", 30, "user")]
    assert by_kind["table"] == [("srbd13", 30, "table"), ("srbd37", 20, "table")]
    r = qc.KEY_CASES["srbd13-range"]
    assert (r.B, r.first, r.count) == (64, 5, 50)
    assert all(c.slots == 4 < c.count and c.B == (16 if c.name == "lip30-N64" else 64 if c.kind == "range" else 48) for c in qc.KEY_CASES.values())
    assert [qc.KEY_CASES[n].wps for n in ("srbd13-N30-w1", "srbd13-N30-w2")] == [1, 2]
    assert set(qc.MEASURED) == set(KEYS)
    assert qc.KEY_RTOL == 1e-9 and qc.SEPARATION == 1e-6 and qc.C_CAPS == (300, 257, 256, 200)


@pytest.mark.parametrize("name", KEYS)
def test_the_keys_are_separated_and_both_oracle_builds_order_alike(name):
    c = qc.KEY_CASES[name]
    J, Jf = qc.initial_costs(name, "off"), qc.initial_costs(name, "fast")
    k, kf = qc.order2_reference(J), qc.order2_reference(Jf)
    live = k[c.first:c.first + c.count]
    sep = qc.separation(live)
    print(f"{name}: J0 {J[np.isfinite(J)].min():.4e} .. {J[np.isfinite(J)].max():.4e}, smallest distance of two keys {sep:.2e} of max |J0|")
    assert sep >= qc.SEPARATION
    assert 0.5 * qc.MEASURED[name]["sep"] <= sep <= 2.0 * qc.MEASURED[name]["sep"]
    np.testing.assert_array_equal(qc.reference_order(k, c.first, c.count), qc.reference_order(kf, c.first, c.count))
    np.testing.assert_allclose(Jf[np.isfinite(J)], J[np.isfinite(J)], rtol=1e-12)
    bad = np.flatnonzero(~np.isfinite(J)).tolist()
    assert bad == ([qc.NAN_AT, qc.INF_AT] if c.kind == "nonfinite" else [])
    if bad:                                                   # a NaN and an overflow, and both builds say so
        assert np.isnan(J[qc.NAN_AT]) and np.isposinf(J[qc.INF_AT]) and np.isnan(Jf[qc.NAN_AT]) and np.isposinf(Jf[qc.INF_AT])
        assert qc.assert_follows(qc.reference_order(k, 0, c.B), k, 0, c.B, qc.key_tol(J)) == 1      # the one declared tie
    else:                                                     # the tolerance hides nothing: no pair of the reference order is inside it
        assert qc.assert_follows(qc.reference_order(k, c.first, c.count), k, c.first, c.count, qc.key_tol(J)) == 0
    if c.kind == "range":                                     # the instances outside hold other warm starts: other keys
        assert len(np.unique(k)) == c.B


@pytest.mark.parametrize("name", KEYS)
def test_a_wrong_key_or_a_wrong_sort_would_show(name):
    c = qc.KEY_CASES[name]
    k = qc.order2_reference(qc.initial_costs(name))
    mut = qc.mutants(name)
    want = {"ascending", "no_terminal"}
    if c.kind == "horizon" and c.N >= 64:
        want.add("one_trip")
    if c.build == "table":
        want.add("handle_consts")
    if c.build in ("x", "friction", "bound", "user"):
        want.add("plain_build")
    if c.first:
        want.add("range_swapped")
    assert set(mut) == want == set(qc.MEASURED[name]) - {"sep"} | {"ascending"}
    share = {m: qc.moved_share(k, v, c.first, c.count) for m, v in mut.items()}
    print(f"{name}: share of the queue positions moved: " + ", ".join(f"{m} {s:.2f}" for m, s in share.items()))
    for m, s in share.items():
        assert s >= qc.MUTATION_SHARE, (m, s)
        if m != "ascending":
            assert abs(s - qc.MEASURED[name][m]) <= 0.005, (m, s)
    assert share["ascending"] >= 0.95


def test_the_numpy_sum_of_the_user_case_is_the_c_oracles_without_the_rows():
    """the one J0 that is not the C oracle's: oracle.ddp.total_cost, checked against the C oracle on the same batch and plain model"""
    name = "srbd13-user"
    c, s = qc.KEY_CASES[name], qc.start(name)
    m = omodels.make_model(c.model, s["csts"][0])
    xs = s["xs"].copy(); xs[:, 0] = s["x0"]
    J_np = np.array([oddp.total_cost(m, xs[b], s["us"][b], s["plain"][1][b]) for b in range(c.B)])
    np.testing.assert_allclose(J_np, qc.mutants(name)["plain_build"], rtol=1e-12)
    assert np.all(qc.initial_costs(name) > J_np)              # the rows add cost on every instance


# ---- the rules themselves -----------------------------------------------------------------------------------------------------------
def test_assert_follows_rejects_what_it_must_and_counts_ties():
    keys = np.array([9.0, 5.0, 7.0, 7.0, 1.0, np.inf, np.inf, 3.0])
    good = np.array([5, 6, 0, 2, 3, 1, 7, 4])
    assert qc.assert_follows(good, keys, 0, 8, 0.0) == 2                                   # inf inf, 7 7
    assert qc.assert_follows(good[[1, 0, 2, 4, 3, 5, 6, 7]], keys, 0, 8, 0.0) == 2         # ties in either order
    assert qc.assert_follows(good, keys, 0, 8, 2.0) == 2 + 4                               # 9 7, 7 5, 5 3, 3 1 fall inside 2
    with pytest.raises(AssertionError, match="rises"):
        qc.assert_follows(good[[0, 1, 2, 3, 4, 6, 5, 7]], keys, 0, 8, 0.0)                 # a swapped pair: 3 before 5
    assert qc.assert_follows(good[[0, 1, 2, 3, 4, 6, 5, 7]], keys, 0, 8, 2.0) == 4         # ... which a tolerance of 2 lets pass
    with pytest.raises(AssertionError, match="missing"):
        qc.assert_follows(np.array([5, 6, 0, 2, 2, 1, 7, 4]), keys, 0, 8, 0.0)
    with pytest.raises(AssertionError, match="outside"):
        qc.assert_follows(np.array([5, 6, 0, 2, 3, 1, 8, 4]), keys, 0, 8, 0.0)
    with pytest.raises(AssertionError, match="entries"):
        qc.assert_follows(good[:7], keys, 0, 8, 0.0)
    # a range: absolute indices, keys by absolute index
    assert qc.assert_follows(np.array([5, 6, 2, 3, 7, 4]), keys, 2, 6, 0.0) == 2
    with pytest.raises(AssertionError, match="outside"):
        qc.assert_follows(np.array([5, 6, 0, 2, 3, 7]), keys, 2, 6, 0.0)
    with pytest.raises(AssertionError, match="outside"):
        qc.assert_follows(np.array([3, 4, 0, 1, 5, 2]), keys, 2, 6, 0.0)                   # relative indices where absolute ones belong
    np.testing.assert_array_equal(qc.reference_order(keys, 2, 6), [5, 6, 2, 3, 7, 4])


def test_order1_keys_are_the_clamp():
    def literal(h):                                           # the bin of queue_order_kernel, transcribed
        return 257 if h < 0 else (256 if h > 256 else h)
    it = np.array([-1, 0, 256, 257, 300, 1, 100])
    np.testing.assert_array_equal(qc.order1_keys(it), [literal(int(h)) for h in it])
    np.testing.assert_array_equal(qc.order1_keys(it), [257, 0, 256, 256, 256, 1, 100])
    assert qc.order1_ties(qc.order1_keys(it)) == 2


def test_order2_reference_and_order3_keys_are_the_documented_formulas():
    J = np.array([4.0e3, np.nan, -np.inf, np.inf, 2.5e4, 7.0, 7.0])
    np.testing.assert_array_equal(qc.order2_reference(J), [4.0e3, np.inf, np.inf, np.inf, 2.5e4, 7.0, 7.0])
    labels = np.array([0, 1, 2, 2, -1, 1, 3])
    s, n = np.array([48.0, 21.0, 10.0, 0.0]), np.array([3.0, 2.0, 1.0, 0.0])
    k = qc.order3_keys(J, labels, s, n)
    tie = lambda j: 1e-3 * j / (abs(j) + 1e9)                                                # noqa: E731
    assert k[0] == 16.0 + tie(4.0e3) and k[5] == 10.5 + tie(7.0)
    assert np.isposinf(k[1:4]).all()                                                        # a non-finite j0 stays the key
    assert k[4] == 1e6 + tie(2.5e4) and k[6] == 1e6 + tie(7.0)                              # unlabelled; a class without history
    assert qc.order3_keys(J, np.array([0, 1, 2, 2, 9, 1, 3]), s, n)[4] == k[4]               # a label outside the table
    # the resolution the module docstring states: one ulp of the key, in units of J0
    for mean, res in ((16.0, 3.6e-3), (8.0, 1.8e-3), (1e6, 116.0)):
        got = np.spacing(mean) * 1e9 ** 2 / 1e6
        assert abs(got - res) <= 0.02 * res, (mean, got)
        j = np.array([1e5, 1e5 + 3.0 * got, 1e5 + 0.2 * got])
        kk = qc.order3_keys(j, np.zeros(3, int), np.array([mean]), np.array([1.0])) if mean < 1e6 else qc.order3_keys(j, -np.ones(3, int), s, n)
        assert kk[1] > kk[0] and abs(kk[2] - kk[0]) <= qc.order3_tol(kk)                     # three ulps apart: ordered; a fifth: a tie
        assert qc.order3_ties(kk, 0, 3) == 1


# ---- order 1, case (c): the oracle needs more than 300 iterations, so every cap is the iteration count --------------------------------
def test_case_c_every_cap_binds_on_the_oracle():
    for v in ("off", "fast"):
        it = qc.c_oracle_iters(qc.C_FREE_MAX_ITERS, v)
        print(f"case (c), build {v}: {it.min()} .. {it.max()} iterations without a binding cap")
        assert (it.min(), it.max()) == qc.C_ITERS_FREE and it.min() > max(qc.C_CAPS)
        for i, cap in enumerate(qc.C_CAPS):
            assert (qc.c_oracle_iters(cap, v, i * qc.C_RANGE, qc.C_RANGE) == cap).all()
    keys = qc.order1_keys(np.repeat(qc.C_CAPS, qc.C_RANGE))
    assert keys.tolist() == [256] * 36 + [200] * 12 and qc.order1_ties(keys) == 46


# ---- order 3: the shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(qc.ORDER3))
def test_order3_shapes_have_classes_to_order_and_a_tie_break_to_see(model):
    s = qc.order3_start(model)
    J, lab, B3 = s["J0"], s["labels"], qc.ORDER3[model][1]
    present, n = np.unique(lab, return_counts=True)
    assert lab.min() >= 0 and lab.max() < s["n_classes"] and len(present) >= 6 and n.max() >= 3
    # inside every class the initial costs are further apart than the tie-break resolves at a mean below 32 (module docstring)
    gap = min(np.diff(np.sort(J[lab == c])).min() for c in present[n > 1])
    print(f"{model}: {len(present)} classes, largest {n.max()}; J0 {J.min():.4e} .. {J.max():.4e}; smallest distance inside a class {gap:.3e}")
    assert gap >= 1e3 * 3.6e-3
    # with a history (one solve per instance, made-up iteration counts below 32) the documented keys have no tie at all ...
    hist = np.zeros((s["n_classes"], 2))
    for c, m in zip(present, n):
        hist[c] = (m * (5 + c % 23) + c % 3, m)
    k = qc.order3_keys(J, lab, hist[:, 0], hist[:, 1])
    assert qc.order3_ties(k, 0, B3) == 0
    # ... a sort by the class mean alone, or in ascending order, is another queue
    mean_only = k - 1e-3 * J / (np.abs(J) + 1e9)
    assert qc.moved_share(k, mean_only, 0, B3) >= qc.MUTATION_SHARE and qc.moved_share(k, -k, 0, B3) >= 0.95
    # case (e): the unlabelled instances and the class without history lead, at 1e6, where the tie-break resolves 116 in J0
    learning, final, unseen = qc.order3_labels_e(model)
    lead = (final < 0) | (final == unseen)
    assert (learning[lead] == -1).all() and (learning[~lead] == final[~lead]).all() and (final == unseen).sum() >= 3
    h = hist.copy(); h[unseen] = 0
    ke = qc.order3_keys(J, final, h[:, 0], h[:, 1])
    assert (ke[lead] > 9e5).all() and (ke[~lead] < 40).all()
    ties = qc.order3_ties(ke, 0, B3)
    close = int((np.diff(np.sort(J[lead])) <= 2 * 116.0).sum())
    print(f"{model} (e): {int(lead.sum())} instances lead; {ties} declared ties among them ({close} pairs of them closer than 232 in J0)")
    assert ties <= close
