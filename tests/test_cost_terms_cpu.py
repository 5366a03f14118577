"""The cost breakdown stated twice in numpy (tests/cost_terms_cases.py: A masks the gains, B groups the rows of the residual) and what
the record promises, checked on the CPU statements; no GPU.  The A-versus-B disagreement per family is the yardstick of the GPU test's
tolerance and is committed as profiles/cost_terms/cpu_disagreement.json:

    python tests/test_cost_terms_cpu.py          # writes that file (write_disagreement)
"""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
from oracle import models as omodels  # noqa: E402
from tests import cost_terms_cases as cc  # noqa: E402

DISAGREEMENT = os.path.join(ROOT, "profiles", "cost_terms", "cpu_disagreement.json")
SHAPES = [(name, kind, N) for name, kind in cc.KINDS for N in (3, 5)]


def write_disagreement(path=DISAGREEMENT):
    with open(path, "w") as f:
        json.dump(cc.measure(), f, indent=1)
        f.write("\n")


@pytest.mark.parametrize("name,kind,N", SHAPES)
def test_the_two_statements_agree_and_the_families_sum_to_the_total(name, kind, N):
    cst, x, u, P = cc.random_case(name, kind, N, 0)
    a, b = cc.statement_a(name, cst, x, u, P), cc.statement_b(name, cst, x, u, P)
    d = cc.relative_disagreement(a, b)
    print(f"{name} {kind} N = {N}: largest relative A - B {d.max():.3e}")
    assert d.max() <= 8 * cc.EPS                    # two sums of the same squares: a few roundings of the record's own size
    for rec, nodes in (a, b):
        fam = rec[1:1 + cc.FAMILIES]
        assert abs(fam.sum() - rec[cc.TOTAL]) <= 14 * cc.EPS * np.abs(fam).sum()
        assert rec.tobytes() == cc.record_of(nodes).tobytes() and rec[cc.NODES] == N
        assert rec[cc.LARGEST] == np.argmax(fam[:12])
    # every family the build has is exercised
    have = {"plain": [0, 1, 2, 4, 5, 6, 12], "x": [0, 1, 2, 4, 5, 6, 11, 12], "bar": [0, 1, 2, 4, 5, 6, 9, 12], "box": [0, 1, 2, 4, 5, 6, 10, 12]}[kind]
    if name == "lip30":
        have = [0, 1, 3, 6, 7, 8]
    elif name != "srbd13":
        have = have + [3, 8]
    assert all(a[0][1 + f] > 0.0 for f in have) and all(a[0][1 + f] == 0.0 for f in range(cc.FAMILIES) if f not in have), a[0]


def test_the_measured_disagreement_is_the_committed_yardstick():
    got = cc.measure()
    with open(DISAGREEMENT) as f:
        want = json.load(f)
    assert list(want) == ["total"] + list(cc.NAMES)
    print(json.dumps(got))
    for k, v in got.items():                        # the committed figure bounds what this machine measures (eps: the floor the GPU test uses)
        assert v <= max(want[k], cc.EPS), (k, v, want[k])


@pytest.mark.parametrize("name,kind", [("srbd37", "x"), ("lip30", "plain"), ("srbd13", "bar")])
def test_a_gain_scales_its_family_alone(name, kind):
    cst, x, u, P = cc.random_case(name, kind, 3, 1)
    ref, _ = cc.statement_a(name, cst, x, u, P)
    for f, gain in enumerate(cc.GAINS):
        if ref[1 + f] == 0.0:
            continue                                # the model has no such term
        # x 4: sqrt(4 g) = 2 sqrt(g) exactly, so the oracle's residuals scale exactly; x 2 goes through sqrt(2) and is held to 4 eps
        for factor, slack in ((4.0, 0.0), (2.0, 4 * cc.EPS)):
            rec, _ = cc.statement_a(name, dataclasses.replace(cst, **{gain: factor * getattr(cst, gain)}), x, u, P)
            assert abs(rec[1 + f] - factor * ref[1 + f]) <= slack * abs(rec[1 + f]), (gain, factor)
            others = [c for c in range(1, 1 + cc.FAMILIES) if c != 1 + f]
            assert rec[others].tobytes() == ref[others].tobytes(), (gain, factor)
        rec, nodes = cc.statement_a(name, dataclasses.replace(cst, **{gain: 0.0}), x, u, P)
        assert rec[1 + f] == 0.0 and np.all(nodes[:, 1 + f] == 0.0), gain


@pytest.mark.parametrize("name,kind", cc.KINDS)
def test_which_families_live_at_the_first_and_the_last_node(name, kind):
    N = 3
    cst, x, u, P = cc.random_case(name, kind, N, 0)
    for _, nodes in (cc.statement_a(name, cst, x, u, P), cc.statement_b(name, cst, x, u, P)):
        stage_only = [4, 5, 6, 7, 8, 9, 10]         # min_f, force_switch, min_qddot, zmp_tracking, constraints and the barriers: 0 at k = N
        state_only = [0, 1, 2, 3, 12]               # the tracking families, rel_pos and the orientation term: 0 at k = 0
        assert np.all(nodes[N, [1 + f for f in stage_only]] == 0.0)
        assert np.all(nodes[0, [1 + f for f in state_only]] == 0.0)


def test_a_nan_reaches_every_family():
    cst, x, u, P = cc.random_case("srbd13", "plain", 3, 0)
    x = x.copy()
    x[2, 4] = np.nan
    rec, nodes = cc.statement_a("srbd13", cst, x, u, P)
    assert np.isnan(rec[:cc.COLS]).all() and rec[cc.LARGEST] == -1 and np.isnan(nodes[2]).all() and not np.isnan(nodes[[0, 1, 3]]).any()


def test_row_families_cover_every_row_of_the_user_row_wrapper():
    cst, x, u, P = cc.random_case("srbd37", "x", 3, 0)
    m = omodels.make_model("srbd37", cst)
    assert isinstance(m, omodels.WithLinearRows)
    assert list(cc.row_families(m, False, 0, P[0])[-1:]) == [11] and list(cc.row_families(m, True, 3, P[3])[-2:]) == [11, 11]


def test_the_binding_declares_the_four_entry_points_and_the_library_names_the_families():
    from srbd_horizon_amd import _lib
    assert {"sddp_cost_terms_words", "sddp_cost_terms_name", "sddp_cost_terms_range_device", "sddp_cost_terms"} <= set(_lib.SYMBOLS)
    _lib.build()
    _lib.load()                                     # (no device needed: the names are static strings)
    assert _lib.COST_TERM_NAMES == cc.NAMES and len(set(cc.NAMES)) == cc.FAMILIES
    assert (_lib.COST_TERMS_WORDS, _lib.COST_TERMS_COLS) == (cc.WORDS, cc.COLS)


if __name__ == "__main__":
    write_disagreement()
    print(open(DISAGREEMENT).read())
