"""Iteration log (include/sddp.h): one record per line search of every solve, kept on the device.

Inputs, cut points and slot counts are those of tests/resume_cases.py; the settings and the instances left out of the oracle
comparison are those of tests/iteration_log_cases.py, decided on the C oracle by tests/test_iteration_log_cpu.py.  Comparisons between
GPU results are `==` on raw bytes.  Against the oracle's trace: record count, accepted alpha, theta, candidates tried and the
iteration count exact; J, accepted J and gap rel 1e-9, mu rel 1e-12, rho RHO_RTOL (tests/parity.py, the same quantities);
expected, A1, B2 within MODEL_RTOL |value| + COST_RTOL |J| (iteration_log_cases: reasoning and the oracle's own scatter).

Test 1 as the issue words it asks that the record after the one of iteration k carries stats.rho of the solve cut at k.  A record
holds rho as the oracle's trace does, AFTER the sweep's update rho = max(rho, 2 max(A1, A1 + B2, 0) / gap), and a solve cut at k has
not run that sweep; so the test asserts the one value the rule allows: stats.rho where the gaps are closed, and the maximum above --
formed from the record's own A1, B2, gap, which is exact in IEEE doubles -- where they are open.  That asks no less."""
import numpy as np
import pytest
import torch

from tests import iteration_log_cases as lc, options_cases as oc, resume_cases as rc
from tests.gpu_support import continue_to as _continue, cut as _solve, log_engine as _engine, log_of as _log, logged as full, used_rows as _used

pytestmark = pytest.mark.gpu
F = lc.F
BUILDS = [("srbd13", 1), ("srbd13", 2), ("srbd37", 1), ("srbd37", 2), ("lip30", 1), ("lip30", 2), ("srbd61", 1)]


# ---- 1. a prefix is a prefix ------------------------------------------------------------------------------------------------------
def _starts_where_the_cut_solve_stopped(q, st, i):
    """record q is the first search from the iterate whose stats are st[i]: J and gap bit for bit, rho as the update rule makes it
    from st.rho and the record's own A1, B2, gap (module docstring).  -> whether rho grew"""
    assert q[F["J"]].tobytes() == st["cost"][i].tobytes() and q[F["gap"]].tobytes() == st["gap"][i].tobytes(), i
    rho = st["rho"][i]
    if q[F["gap"]] > 0.0:
        rho = max(rho, 2.0 * max(max(q[F["A1"]], q[F["A1"]] + q[F["B2"]]), 0.0) / q[F["gap"]])
    assert q[F["rho"]].tobytes() == np.float64(rho).tobytes(), (i, q[F["rho"]], st["rho"][i], rho)
    return rho > st["rho"][i]


@pytest.mark.parametrize("model,wps", BUILDS)
@pytest.mark.parametrize("case", ["base", "A"])
def test_the_records_are_the_stats_of_the_solve_cut_at_every_k(model, wps, case):
    b = rc.batch(model)
    _, _, st_full, rec, n = full(model, case, wps)
    eng = _engine(model, case, wps, rows=0, resume=False)              # the ordinary kernels, one launch per prefix
    checked = nxt = grown = 0
    for k in range(0, 9):
        st = _solve(eng, b, k)[2]
        for i in range(len(st)):
            r = rec[i, :n[i]]
            if k == 0:                                                   # max_iters = 0: the starting point, which the first search starts from
                assert st["iters"][i] == 0 and st["rho"][i] == 0.0 and st["rollouts"][i] <= 1, i
                if n[i]:
                    grown += _starts_where_the_cut_solve_stopped(r[0], st, i)
                    assert r[0, F["iters"]] == (1.0 if r[0, F["alpha"]] > 0.0 else 0.0), i
                    nxt += 1
                continue
            if st["iters"][i] != k:
                continue
            row = np.flatnonzero((r[:, F["iters"]] == k) & (r[:, F["alpha"]] > 0.0))
            assert len(row) == 1, (i, k, r[:, F["iters"]])
            j = row[0]
            assert r[j, F["J_accepted"]].tobytes() == st["cost"][i].tobytes() and r[j, F["alpha"]].tobytes() == st["alpha"][i].tobytes(), (i, k)
            assert r[j, F["rollouts"]] == st["rollouts"][i] and r[j, F["mu_bumps"]] >= 0 and r[j, F["reserved"]] == 0.0, (i, k)
            checked += 1
            if j + 1 < n[i]:
                grown += _starts_where_the_cut_solve_stopped(r[j + 1], st, i)
                nxt += 1
    eng.close()
    first = rec[:, 0]
    assert (first[n > 0][:, F["J"]] != 0.0).all()
    print(f"{model} w{wps} {case}: {checked} records checked against a prefix, {nxt} successors, rho grown in {grown}")
    assert checked >= len(n) and nxt >= len(n)
    assert (rec[np.arange(len(n)), np.maximum(n - 1, 0), F["iters"]][n > 0] == st_full["iters"][n > 0]).all()
    assert (rec[np.arange(len(n)), np.maximum(n - 1, 0), F["rollouts"]][n > 0] == st_full["rollouts"][n > 0]).all()


# ---- 2. against the oracle's trace ------------------------------------------------------------------------------------------------
ORACLE = [(m, c, w) for m, w in BUILDS for c in lc.SETTINGS if not (m != "srbd13" and c in ("T",))]


@pytest.mark.parametrize("model,case,wps", ORACLE)
def test_the_records_are_the_oracles_trace(model, case, wps):
    b = lc.batch(model, case)
    if model == "srbd13" and case == "ir1":                               # its own seeds (iteration_log_cases.IR1_SEEDS)
        eng = _engine(model, case, wps)
        _solve(eng, b)
        rec, n = _log(eng)
        eng.close()
    else:
        rec, n = full(model, case, wps)[3:]
    tr = lc.traces(model, case)[0]
    left_out = lc.excluded(model, case)
    worst = {}
    for i in range(len(n)):
        if i in left_out:
            continue
        o, g = tr[i], rec[i, :n[i]]
        assert n[i] == len(o), (i, n[i], len(o))
        for f in ("alpha", "theta", "tried"):
            np.testing.assert_array_equal(g[:, F[f]], o[:, F[f]], err_msg=f"instance {i} {f}")
        acc = np.cumsum(o[:, F["alpha"]] > 0.0)
        np.testing.assert_array_equal(g[:, F["iters"]], acc, err_msg=f"instance {i} iters")
        for f, tol in (("J", lc.COST_RTOL), ("J_accepted", lc.COST_RTOL), ("gap", 1e-9), ("mu", 1e-12), ("rho", oc.RHO_RTOL)):
            d = np.abs(g[:, F[f]] - o[:, F[f]])
            lim = tol * np.abs(o[:, F[f]])
            worst[f] = max(worst.get(f, 0.0), float((d / np.maximum(lim, 1e-300)).max()) if len(d) and d.max() > 0 else 0.0)
            assert (d <= lim).all(), (i, f, g[:, F[f]], o[:, F[f]])
        for f in ("expected", "A1", "B2"):
            d = np.abs(g[:, F[f]] - o[:, F[f]])
            lim = lc.MODEL_RTOL * np.abs(o[:, F[f]]) + lc.COST_RTOL * np.abs(o[:, F["J"]])
            worst[f] = max(worst.get(f, 0.0), float((d / lim).max()) if len(d) else 0.0)
            assert (d <= lim).all(), (i, f, g[:, F[f]], o[:, F[f]])
    print(f"{model} w{wps} {case}: records {n.tolist()}; largest difference as a fraction of its bound {worst}")


# ---- 3. slots are not instances -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 2])
def test_the_log_does_not_depend_on_slots_or_queue_order(order):
    model = "srbd13"
    b, B = rc.batch(model), rc.SHAPES[model][1]
    ref = full(model, "base", 2)
    eng = _engine(model, "base", 2, queue_order=order)
    _solve(eng, b)
    assert eng.queue_info()[1:] == (rc.MAX_SLOTS[model], B)
    few = _log(eng)
    eng.close()
    eng = _engine(model, "base", 2, max_slots=B)
    _solve(eng, b)
    assert eng.queue_info()[2] == 0                                      # no queue: instance b on slot b
    wide = _log(eng)
    eng.close()
    for got in (few, wide):
        assert (got[1] == ref[4]).all() and _used(*got) == _used(ref[3], ref[4])
    assert few[0].tobytes() == wide[0].tobytes()


def test_a_range_launch_leaves_the_other_instances_records_alone():
    model = "srbd13"
    b, B = rc.batch(model), rc.SHAPES[model][1]
    eng = _engine(model, "A", 2)
    _solve(eng, b)                                                       # pre-fill: every instance holds the records of set A
    before = _log(eng)
    assert (before[1] > 8).all()
    eng.set_options(alpha_0=1.0)                                         # the range is solved again under the base options: fewer records
    eng.load(b["x0"], b["xs"], b["us"])
    P = torch.from_numpy(b["params"].copy()).to("cuda:0")
    eng.solve_range_device(P, 16, 16)
    after = _log(eng)
    eng.close()
    inside = np.zeros(B, dtype=bool); inside[16:32] = True
    ref = full(model, "base", 2)
    assert after[0][~inside].tobytes() == before[0][~inside].tobytes() and (after[1][~inside] == before[1][~inside]).all()
    assert (after[1][inside] == ref[4][inside]).all()
    assert _used(after[0][inside], after[1][inside]) == _used(ref[3][inside], ref[4][inside])
    for i in np.flatnonzero(inside):                                     # the rows beyond the new count keep the older solve's records
        assert after[0][i, after[1][i]:].tobytes() == before[0][i, after[1][i]:].tobytes()


# ---- 4. cut and continue ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,case,wps", [("srbd13", "base", 1), ("srbd13", "A", 2), ("srbd13", "E", 2), ("srbd13", "T", 1), ("srbd13", "ir1", 2),
                                            ("srbd37", "base", 1), ("srbd37", "A", 2), ("lip30", "E", 2), ("srbd61", "base", 1)])
def test_cut_and_continued_gives_the_log_of_the_uncut_solve(model, case, wps):
    b, ref = rc.batch(model), full(model, case, wps)
    eng = _engine(model, case, wps)
    at_cut = _solve(eng, b, rc.CUT[model])
    log_cut = _log(eng)
    done = at_cut[2]["status"] != 1
    assert (~done).any()
    two = _continue(eng, rc.TOTAL)
    log_two = _log(eng)
    k1, k2 = rc.CUTS3[model]
    _solve(eng, b, k1); _continue(eng, k2); three = _continue(eng, rc.TOTAL)
    log_three = _log(eng)
    eng.close()
    for got, lg in ((two, log_two), (three, log_three)):
        assert got[2].tobytes() == ref[2].tobytes() and got[0].tobytes() == ref[0].tobytes()
        assert (lg[1] == ref[4]).all() and _used(*lg) == _used(ref[3], ref[4])
    # an instance that finished in the first slice: the continue launch left its records and count alone
    assert log_two[0][done].tobytes() == log_cut[0][done].tobytes() and (log_two[1][done] == log_cut[1][done]).all()
    # an unfinished one had written the records of its first slice (one that then ends at the convergence test adds none)
    assert (log_cut[1][~done] <= ref[4][~done]).all() and (log_cut[1][~done] < ref[4][~done]).any()
    assert _used(log_cut[0][~done], log_cut[1][~done]) == [ref[3][i, :log_cut[1][i]].tobytes() for i in np.flatnonzero(~done)]


# ---- 5. saturation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,wps", [("srbd13", 2), ("srbd37", 1)])
def test_a_full_log_stops_at_its_rows_and_stays_inside_them(model, wps):
    b, ref, B = rc.batch(model), full(model, "base", wps), rc.SHAPES[model][1]
    rows = 5                                                            # between the shortest solve and the longest (asserted below)
    eng = _engine(model, "base", wps, rows=rows)
    rec_d, n_d = eng.iteration_log_device()
    assert rec_d.shape == (B, rows, 16) and n_d.shape == (B,) and eng.device_buffer(9)[1] == B * rows * 16 * 8
    guard = -(1.0 + np.arange(B * rows * 16, dtype=np.float64)).reshape(B, rows, 16)
    _log(eng)                                                           # (waits for the stream: the buffers have been zeroed)
    rec_d.copy_(torch.from_numpy(guard).to(rec_d.device))              # every row of every instance holds a pattern
    torch.cuda.synchronize()
    out = _solve(eng, b)
    rec, n = _log(eng)
    torch.cuda.synchronize()
    assert rec_d.cpu().numpy().tobytes() == rec.tobytes() and (n_d.cpu().numpy() == n).all()
    eng.close()
    assert out[2].tobytes() == ref[2].tobytes()
    assert (ref[4] > rows).any() and (ref[4] < rows).any() and (n == np.minimum(ref[4], rows)).all()
    for i in range(B):
        assert rec[i, :n[i]].tobytes() == ref[3][i, :n[i]].tobytes(), i
        assert rec[i, n[i]:].tobytes() == guard[i, n[i]:].tobytes(), i        # rows not written keep the pattern: the neighbour's too
    short = np.flatnonzero(n < rows)
    assert any(i + 1 < B and n[i + 1] == rows for i in short) and any(i > 0 and n[i - 1] == rows for i in short)   # pattern rows beside full logs
    # a continue launch on a full log writes nothing either
    eng = _engine(model, "base", wps, rows=rows)
    _solve(eng, b, rc.CUT[model]); _continue(eng, rc.TOTAL)
    rec2, n2 = _log(eng)
    eng.close()
    assert (n2 == n).all() and _used(rec2, n2) == _used(rec, n)


# ---- 6. constants table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,wps", [("srbd13", 1), ("srbd37", 2)])
def test_a_table_of_the_handles_own_constants_gives_the_same_log(model, wps):
    b, ref, B = rc.batch(model), full(model, "base", wps), rc.SHAPES[model][1]
    eng = _engine(model, "base", wps)
    eng.set_instance_consts({"m": np.full(B, eng.consts.m)})
    assert eng.instance_consts_active()
    out = _solve(eng, b)
    rec, n = _log(eng)
    eng.close()
    assert out[2].tobytes() == ref[2].tobytes() and rec.tobytes() == ref[3].tobytes() and (n == ref[4]).all()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_the_log_is_refused_where_it_cannot_work():
    model = "srbd13"
    b = rc.batch(model)
    ref = full(model, "base", 1)
    eng = _engine(model, "base", rows=0, resume=False)
    with pytest.raises(RuntimeError, match="sddp_enable_resume"):
        eng.enable_iteration_log(8)
    with pytest.raises(RuntimeError, match="sddp_enable_iteration_log"):
        eng.device_buffer(9)
    with pytest.raises(RuntimeError, match="sddp_enable_iteration_log"):
        eng.device_buffer(10)
    with pytest.raises(RuntimeError, match="sddp_enable_iteration_log"):
        eng.iteration_log()
    assert _solve(eng, b)[2].tobytes() == ref[2].tobytes()
    eng.enable_resume()
    for rows in (-1, 4097):
        with pytest.raises(RuntimeError, match="rows must be 1 .. 4096"):
            eng.enable_iteration_log(rows)
    assert eng.iteration_log_rows() == 0
    assert _solve(eng, b)[2].tobytes() == ref[2].tobytes()
    eng.enable_iteration_log(4096)
    assert eng.iteration_log_rows() == 4096
    eng.enable_iteration_log(0)
    with pytest.raises(RuntimeError, match="sddp_enable_iteration_log"):
        eng.device_buffer(9)
    eng.enable_iteration_log(8)
    eng.enable_resume(False)                                             # the log goes with the resumable kernels
    assert eng.iteration_log_rows() == 0
    assert _solve(eng, b)[2].tobytes() == ref[2].tobytes()
    eng.close()
    rows_x = [dict(a=[1.0] + [0.0] * 18, w=1e-6, kind="state")]
    bx = dict(b, params=np.concatenate([b["params"], np.zeros(b["params"].shape[:2] + (8,))], axis=2))      # the user rows' reference columns
    for kw, bb in ((dict(consts=dict(b["consts"], friction_barrier_weight=1e-3)), b), (dict(second_order=2), b),
                   (dict(consts=dict(b["consts"], extra_rows=rows_x)), bx)):
        untouched = _engine(model, "base", rows=0, resume=False, **kw)
        want = _solve(untouched, bb)
        untouched.close()
        eng = _engine(model, "base", rows=0, resume=False, **kw)
        with pytest.raises(RuntimeError, match="plain builds only"):
            eng.enable_iteration_log(8)
        with pytest.raises(RuntimeError, match="sddp_enable_iteration_log"):
            eng.device_buffer(9)
        got = _solve(eng, bb)
        eng.close()
        assert (want[2]["status"] != 3).all()
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), kw


# ---- 8. nothing else moves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,wps", BUILDS)
def test_a_logged_solve_returns_the_bytes_of_an_ordinary_one(model, wps):
    b = rc.batch(model)
    eng = _engine(model, "base", wps, rows=0, resume=False)
    plain = _solve(eng, b)
    eng.close()
    logged = full(model, "base", wps)
    for got, want, what in zip(logged[:3], plain, ("xs", "us", "stats")):
        assert got.tobytes() == want.tobytes(), what


# ---- poisoned LDS -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,wps", BUILDS)
def test_a_logged_solve_does_not_depend_on_what_the_lds_held(model, wps):
    b, ref = rc.batch(model), full(model, "A", wps)
    eng = _engine(model, "A", wps)
    eng.set_options(max_iters=rc.TOTAL)
    eng.load(b["x0"], b["xs"], b["us"])
    eng.poison_lds()
    eng.solve(b["params"])
    x, u, st = eng.fetch()
    rec, n = _log(eng)
    eng.close()
    assert np.isfinite(x).all() and np.isfinite(rec[:, :, :]).all()
    assert st.tobytes() == ref[2].tobytes() and x.tobytes() == ref[0].tobytes() and (n == ref[4]).all() and _used(rec, n) == _used(ref[3], ref[4])
