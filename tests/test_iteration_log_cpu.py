"""Iteration log without a GPU: the names of the record's words and the build list, the refusals that need no device, and -- on the C oracle alone --
that the settings of tests/iteration_log_cases.py show every kind of record the GPU test compares, and on which instances the
oracle is a stable reference."""
import ctypes as C

import numpy as np

from oracle import cport
from srbd_horizon_amd import _lib
from tests import iteration_log_cases as lc, resume_cases as rc

F = lc.F


def test_the_first_twelve_words_of_a_record_are_the_oracles_trace_record():
    assert list(_lib.LOG_FIELDS[:12]) == ["J", "A1", "B2", "rho", "gap", "expected", "alpha", "J_accepted", "theta", "mu", "tried", "slack"]


def test_the_log_units_are_exactly_the_builds_without_traits():
    units = _lib.translation_units()
    names = [n for n, _ in units if not n.endswith("_inspect")]      # the units of the solve kernels (the others: test_build_table_cpu)
    log = sorted(n[:-len("_log")] for n in names if n.endswith("_log"))
    assert log == sorted(b.fn for b in _lib.INSTANCES if not b.traits) == ["lip30", "srbd13", "srbd37", "srbd61"]
    assert len(set(names)) == len(names) == len(_lib.INSTANCES) + 2 * len(log) == len([n for n in names if not n.endswith("_log")]) + 4
    by_name = dict(units)
    LOG = "-DSDDP_INST_VARIANT=%d" % _lib.VARIANTS.index("log")
    for name, defs in units:
        # a log unit is compiled with its build's own flags and the definition that says it is the log variant; no other unit has that
        assert (LOG in defs) == name.endswith("_log") and len([d for d in defs if d.startswith("-DSDDP_INST_VARIANT")]) <= 1, name
        if name.endswith("_log"):
            assert [d for d in defs if d != LOG] == by_name[name[:-len("_log")]], name
    for unit in ("srbd61", "srbd61_resume", "srbd61_log"):
        assert [d for d in by_name[unit] if not d.startswith("-D")] == ["-mllvm", "-sink-insts-to-avoid-spills"], unit
    assert _lib.compile_command("srbd61_log")[-3:] == ["-mllvm", "-sink-insts-to-avoid-spills", LOG] and LOG == "-DSDDP_INST_VARIANT=2"


def test_calls_without_a_handle_are_argument_errors():
    _lib.build()
    lib = _lib.load()
    rows, words = C.c_int(-1), C.c_int(-1)
    ERR_ARG = -1                                                         # SDDP_ERR_ARG
    assert lib.sddp_enable_iteration_log(None, 8) == ERR_ARG
    assert lib.sddp_iteration_log_info(None, C.byref(rows), C.byref(words)) == ERR_ARG
    assert lib.sddp_fetch_iteration_log(None, 0, 1, None, None) == ERR_ARG
    assert (rows.value, words.value) == (-1, -1)


def _retry_pairs(tr):
    """indices i of a search that failed with theta = 1 and was redone from the same iterate with theta = 0"""
    return [i for i in range(len(tr) - 1) if tr[i, F["alpha"]] == 0.0 and tr[i, F["theta"]] == 1.0 and tr[i + 1, F["theta"]] == 0.0
            and tr[i + 1, F["J"]] == tr[i, F["J"]]]


def test_the_settings_show_every_kind_of_record_on_the_c_oracle():
    """a GPU test of a field nobody exercises proves nothing: (1) a theta-retry pair (setting "T": srbd13 seeds 8, 23, 44 -- not to be
    had from seeds under the five settings of resume_cases, see iteration_log_cases), (2) mu bumped in a sweep (set E), (3) open gaps
    with rho > 0 (set A), (4) a solve that converges with zero records ("Z"), and ladders longer than one step (base: up to 9)."""
    t = lc.traces("srbd13", "T")[0]
    pairs = {b: _retry_pairs(t[b]) for b in range(len(t)) if _retry_pairs(t[b])}
    assert set(pairs) >= {8, 23, 44}, pairs
    for b, idx in pairs.items():      # the redone search is what the iteration goes on with
        assert all(t[b][i + 1, F["alpha"]] > 0.0 for i in idx), b
    assert not any(_retry_pairs(tr) for case in ("base", "A", "E", "so0", "ir1") for tr in lc.traces("srbd13", case)[0])
    for model in rc.SHAPES:
        e = lc.traces(model, "E")[0]
        mu0 = lc.options("E")["mu0"]
        assert all(len(tr) and tr[0, F["mu"]] > max(mu0, 0.0) for tr in e), model             # (2) the first sweep bumps, every instance
        z = lc.traces(model, "Z")
        assert all(len(tr) == 0 for tr in z[0]) and (cport.stat(z[1], "status") == 0).all(), model      # (4)
    for model in ("srbd13", "srbd37", "lip30"):
        a = lc.traces(model, "A")[0]
        assert any(((tr[:, F["gap"]] > 0.0) & (tr[:, F["rho"]] > 0.0)).any() for tr in a), model     # (3)
    grow = [b for b, tr in enumerate(lc.traces("srbd13", "A")[0]) if (np.diff(tr[:, F["rho"]]) > 0.0).any()]
    assert grow, "no srbd13 instance of set A raises rho after its first search"
    assert max(tr[:, F["tried"]].max() for tr in lc.traces("srbd13", "base")[0]) >= 4
    # saturation (rows = 5 in the GPU test: some instances fill their rows, some leave pattern rows) and the cuts have something to cut
    for model in ("srbd13", "srbd37"):
        counts = [len(tr) for tr in lc.traces(model, "base")[0]]
        assert min(counts) < 5 < max(counts), (model, counts)
    assert min(len(tr) for tr in lc.traces("srbd13", "base")[0]) >= 3 and max(len(tr) for tr in lc.traces("srbd13", "base")[0]) > rc.CUT["srbd13"]
    assert max(len(tr) for case in lc.SETTINGS for m in rc.SHAPES for tr in lc.traces(m, case)[0]) < lc.ROWS


def test_the_oracle_is_a_stable_reference_on_all_but_one_instance_in_48():
    """Which instances the GPU test leaves out of the oracle comparison: those on which the oracle's two builds (-ffp-contract=off /
    fast) disagree in the record count or an accepted step length.  At most 1 in 48 for srbd13, none for the other models.  (srbd13
    "ir1" does not meet that on seeds 0..47 -- thirteen instances -- and is compared on iteration_log_cases.IR1_SEEDS.)"""
    worst = {}
    for model, (N, B) in rc.SHAPES.items():
        for case in lc.SETTINGS:
            ex = lc.excluded(model, case)
            assert len(ex) <= (1 if model == "srbd13" else 0), (model, case, ex)
            # the reference's own scatter in the fields compared with a tolerance, in the GPU test's metric (see there)
            a, c = lc.traces(model, case, "off")[0], lc.traces(model, case, "fast")[0]
            for b in set(range(B)) - set(ex):
                for f in ("expected", "A1", "B2"):
                    d = np.abs(a[b][:, F[f]] - c[b][:, F[f]]) / (lc.MODEL_RTOL * np.abs(a[b][:, F[f]]) + lc.COST_RTOL * np.abs(a[b][:, F["J"]]))
                    worst[f] = max(worst.get(f, 0.0), float(d.max()) if d.size else 0.0)
    print("largest off/fast difference of the oracle, as a fraction of the GPU test's bound:", worst)
    assert max(worst.values()) <= 0.1
    assert len(set(lc.IR1_SEEDS)) == 48 and [s for s in range(48) if s not in lc.IR1_SEEDS] == [3, 4, 8, 9, 13, 14, 23, 24, 29, 33, 34, 39, 44]
