"""What the GPU tests share: loading and solving a batch on a handle, cutting and continuing a solve, the byte comparison of two
results, the references several modules compare against (computed once per key, read-only), and the explanation of an instance on
another iteration count than the oracle.  Plain functions, no fixtures; no test module imports another."""
import functools

import numpy as np

from oracle import models as omodels
from srbd_horizon_amd.engine import DdpEngine
from tests import iteration_log_cases as lc, resume_cases as rc

BUILDS = {"srbd13": (1, 2), "srbd37": (1, 2), "lip30": (2,), "srbd61": (1,)}          # waves_per_simd per model


def frozen(arrays):
    """a cached reference: the same arrays, read-only"""
    for a in arrays:
        a.setflags(write=False)
    return arrays


def solve(eng, batch, params=None):
    """load the batch's start, solve (through sddp_solve) -> copies of (x, u, stats)"""
    eng.load(batch["x0"], batch["xs"], batch["us"])
    x, u = eng.solve(batch["params"] if params is None else params)
    return x.copy(), u.copy(), eng.stats.copy()


def snap(eng):
    x, u, st = eng.fetch()
    return x.copy(), u.copy(), st.copy()


def cut(eng, batch, k=rc.TOTAL):
    """a fresh solve of the whole batch with max_iters = k (through sddp_solve: the parameters become the resident tensor)"""
    eng.set_options(max_iters=k)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(batch["params"])
    return snap(eng)


def continue_to(eng, k, first=0, count=None):
    eng.set_options(max_iters=k)
    eng.continue_solve(None, first, count)
    return snap(eng)


def same_bytes(got, ref, sel=slice(None), msg=""):
    """(x, u, stats) twice: the same bytes on the instances `sel`; where the stats differ, the field that does"""
    assert got[0][sel].tobytes() == ref[0][sel].tobytes(), f"xs differ {msg}"
    assert got[1][sel].tobytes() == ref[1][sel].tobytes(), f"us differ {msg}"
    if got[2][sel].tobytes() != ref[2][sel].tobytes():
        for f in ref[2].dtype.names:
            np.testing.assert_array_equal(got[2][f][sel], ref[2][f][sel], err_msg=f"stats.{f} {msg}")
        raise AssertionError(f"stats differ in their padding {msg}")


# ---- the handles and references of tests/resume_cases.py -------------------------------------------------------------------------------
def resume_engine(model, case, wps=1, resume=True, consts=None, **over):
    N, B = rc.SHAPES[model]
    opts = dict(rc.options(case), waves_per_simd=wps, max_slots=rc.MAX_SLOTS[model])
    opts.update(over)
    eng = DdpEngine(model, N, B, opts=opts, consts=rc.batch(model)["consts"] if consts is None else consts)
    if resume:
        eng.enable_resume()
    return eng


@functools.lru_cache(maxsize=None)
def uncut(model, case, wps):
    """the ordinary handle (no sddp_enable_resume) at max_iters = 100: computed once, read-only"""
    eng = resume_engine(model, case, wps, resume=False)
    out = cut(eng, rc.batch(model), rc.TOTAL)
    eng.close()
    return frozen(out)


@functools.lru_cache(maxsize=None)
def cut_ref(model, wps, k):
    """an ordinary handle (no sddp_enable_resume) at max_iters = k: computed once, read-only"""
    if k == rc.TOTAL:
        return uncut(model, "base", wps)
    eng = resume_engine(model, "base", wps, resume=False)
    out = cut(eng, rc.batch(model), k)
    eng.close()
    return frozen(out)


# ---- the logged handles and references of tests/iteration_log_cases.py -----------------------------------------------------------------
def log_engine(model, case, wps=1, rows=lc.ROWS, resume=True, consts=None, **over):
    N, B = rc.SHAPES[model]
    opts = dict(lc.options(case), waves_per_simd=wps, max_slots=rc.MAX_SLOTS[model])
    opts.update(over)
    eng = DdpEngine(model, N, B, opts=opts, consts=lc.batch(model, case)["consts"] if consts is None else consts)
    if resume:
        eng.enable_resume()
    if rows:
        eng.enable_iteration_log(rows)
    return eng


def log_of(eng):
    rec, n = eng.iteration_log()
    return rec.copy(), n.copy()


def used_rows(rec, n):
    """the bytes of the rows in use, instance by instance"""
    return [rec[b, :n[b]].tobytes() for b in range(len(n))]


@functools.lru_cache(maxsize=None)
def logged(model, case, wps):
    """(x, u, stats, records, counts) of the uncut logged solve on seeds 0..B-1 (resume_cases' batch; "Z": restarted), read-only"""
    eng = log_engine(model, case, wps)
    out = cut(eng, lc.batch(model, case) if case == "Z" else rc.batch(model), rc.TOTAL) + log_of(eng)
    eng.close()
    return frozen(out)


# ---- another iteration count than the oracle ---------------------------------------------------------------------------------------------
def explain(c, s, opts, engine_over, idx):
    """the instances on another iteration count than the oracle: one-step shadowing of the GPU path (tests/shadow.py)"""
    from tests import shadow
    recs = shadow.explain_divergent(c.model, c.N, opts, engine_over, s["consts"], omodels.RobotConsts(**s["consts"]), s, idx)
    out = []
    for r in recs:
        try:
            shadow.assert_shadowed(r)
            verdict = "every GPU step is the oracle's step from the same iterate (a step the oracle cannot decide either)"
        except AssertionError:
            verdict = "NOT explained by one-step shadowing: a kernel bug"
        out.append(f"instance {r['instance']}: GPU {r['gpu_iters']} oracle {r['oracle_iters']} / {r['oracle_fast_iters']} iterations; "
                   f"first split {r['split_gpu']}; {verdict}")
    return "\n".join(out)
