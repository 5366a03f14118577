"""What the GPU tests share: loading and solving a batch on a handle, a whole solve compared with the C oracle's (the cases of
tests/whole_solve_cases.py), cutting and continuing a solve, the byte comparison of two results, the references several modules
compare against (computed once per key, read-only), what the plan inspectors' modules share (the contract of DESIGN.md section 5,
"Plan inspectors", as three routines), what the two sensitivities' modules share, and the explanation of an instance on another iteration count than the oracle.  Plain
functions, no fixtures; no test module imports another."""
import functools
from typing import Callable, NamedTuple

import numpy as np
import pytest
import torch

from oracle import models as omodels
from srbd_horizon_amd import _lib, workload
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.fleet import FleetQueue
from tests import iteration_log_cases as lc, parity, plan_audit_cases as pac, resume_cases as rc, whole_solve_cases as wc
from tests.oracle_refs import frozen      # noqa: F401  (a cached reference: the same arrays, read-only)

BUILDS = {"srbd13": (1, 2), "srbd37": (1, 2), "lip30": (2,), "srbd61": (1,)}          # waves_per_simd per model


def dev(a):
    """a float64 CUDA tensor of an array (a tensor, None: itself)"""
    return a if a is None or isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")


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


def whole_solve(name, default_consts=False, check_handle=None, **engine_over):
    """the case of tests/whole_solve_cases.py on a fresh handle (default_consts: one created without constants; check_handle(eng)
    before the solve), compared with the C oracle's solve field by field (parity.assert_matches_c_oracle) -> (x, u, stats)"""
    c, s = wc.CASES[name], wc.start(name)
    eng = DdpEngine(c.model, c.N, len(c.seeds), opts=dict(wc.options(c), **engine_over), consts=None if default_consts else s["consts"])
    if check_handle is not None:
        check_handle(eng)
    x, u, st = solve(eng, s)
    eng.close()
    parity.assert_matches_c_oracle(x, u, st, *wc.oracle(name), explain=lambda idx: explain(c, s, wc.options(c), engine_over, idx))
    return x, u, st


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


# ---- the plan inspectors (audit, stationarity certificate, cost breakdown): what their three test modules share ------------------------------
@functools.lru_cache(maxsize=None)
def solved(model, N, B, kind="plain", seeds=None, wps=None, knots=0):
    """a handle on the problem of a case (tests/plan_audit_cases.py problem) with its solve (and, knots > 0, its policy launch) done, and
    what it gave: (eng, RobotConsts, batch, x, u, stats, P), computed once, arrays read-only"""
    batch, P, consts, opts = pac.problem(model, N, B, kind, seeds)
    eng = DdpEngine(model, N, B, opts=opts if wps is None else dict(opts, waves_per_simd=wps), consts=consts)
    if knots:
        eng.enable_policy(knots)
    x, u, st = solve(eng, batch, P)
    if knots:
        eng.policy_range_device()
    frozen((x, u, st, P))
    return eng, omodels.RobotConsts(**consts), batch, x, u, st, P


class Inspector(NamedTuple):
    name: str               # DdpEngine.<name> and .<name>_device, FleetQueue.<name>, sddp_<name>_range_device
    words: int
    optional: dict          # the optional outputs of <name>_device: keyword -> eng -> trailing shape
    raw: Callable           # (eng, first, count, d_x, d_u, d_out) -> the return value of sddp_<name>_range_device on the whole horizon

    def device(self, eng, first=0, count=None, x=None, u=None, optional=True, **kw):
        """<name>_device on fresh tensors pre-filled with 7.0 -> numpy (records, the optional outputs in their order, None without
        `optional`)"""
        n = eng.B - first if count is None else count
        mk = lambda *shape: torch.full((n, *shape), 7.0, dtype=torch.float64, device="cuda")      # noqa: E731
        out, opt = mk(self.words), {k: mk(*shape(eng)) if optional else None for k, shape in self.optional.items()}
        x, u = dev(x), dev(u)
        torch.cuda.synchronize()      # the fills and uploads are on torch's stream, the kernel on the handle's: torch finishes first
        getattr(eng, self.name + "_device")(out, first, n, x=x, u=u, **opt, **kw)
        eng.synchronize()
        return (out.cpu().numpy(), *(None if t is None else t.cpu().numpy() for t in opt.values()))

    def host(self, eng, first=0, count=None):
        """the records of DdpEngine.<name>, the host-array twin"""
        r = getattr(eng, self.name)(first, count)
        return r["record"] if isinstance(r, dict) else r


AUDIT = Inspector("audit", _lib.AUDIT_WORDS, {},
                  lambda e, f, n, dx, du, out: e.lib.sddp_audit_range_device(e.h, f, n, 0, e.N, dx, du, 0.0, out))
STATIONARITY = Inspector("stationarity", len(_lib.STATIONARITY_FIELDS), dict(lam=lambda e: (e.N + 1, e.nx), grad=lambda e: (e.N, e.nu)),
                         lambda e, f, n, dx, du, out: e.lib.sddp_stationarity_range_device(e.h, f, n, dx, du, out, None, None))
COST_TERMS = Inspector("cost_terms", _lib.COST_TERMS_WORDS, dict(nodes=lambda e: (e.N + 1, _lib.COST_TERMS_COLS)),
                       lambda e, f, n, dx, du, out: e.lib.sddp_cost_terms_range_device(e.h, f, n, dx, du, out, None))


# ---- the two sensitivities (parameter and constant gradient): what their two test modules share, by the Inspector they drive ------------------
def run(insp, eng, first=0, count=None, x=None, u=None, full=True):
    """<name>_device on fresh device tensors -> numpy (record, the per-node output, lambda [n, N + 1, nx]); None for the two without full"""
    return insp.device(eng, first, count, x, u, optional=full)


def engine_with_plan(model, N, B, consts, P, batch, opts=None, solve_it=False):
    """a handle whose last solve launch carried P: at max_iters = 0 (the plan is then the warm start) unless solve_it"""
    eng = DdpEngine(model, N, B, opts=dict(pac.OPTS, **({} if solve_it else dict(max_iters=0)), **(opts or {})), consts=consts)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(P)
    return eng


def assert_same_costates(words, eng, got, x=None, u=None, first=0, count=None):
    """lambda and the record's `words` (|| lambda_0 ||, stationarity, defect) are the stationarity certificate's, bit for bit"""
    srec, slam, _ = STATIONARITY.device(eng, first, count, x, u)
    assert got[2].tobytes() == slam.tobytes()
    assert got[0][:, list(words)].tobytes() == srec[:, [4, 0, 6]].tobytes()


def assert_a_user_build_is_refused(insp, match):
    """a user build (non-linear rows) has no derivative code: RuntimeError `match`, SDDP_ERR_ARG, and the handle still works"""
    from tests import user_terms_defs as ud
    N, B = 20, 2
    spec, mid = ud.user_case("srbd13_terrain", N)
    batch = workload.make_batch("srbd13", N, [0, 1])
    eng = DdpEngine("srbd13", N, B, opts=dict(pac.OPTS, max_iters=0), consts=dict(batch["consts"], extra_rows=spec.extra_rows()), model_id=mid)
    eng.load(batch["x0"], batch["xs"], batch["us"])
    eng.solve(ud.widen(batch["params"], spec))
    out = torch.zeros((B, insp.words), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match=match):
        getattr(eng, insp.name + "_device")(out)
    assert insp.raw(eng, 0, B, None, None, eng._dev(out, out.shape)) == -1      # SDDP_ERR_ARG
    assert STATIONARITY.device(eng)[0].shape == (B, 8)                           # and the handle still works
    eng.close()


def assert_a_nan_stays_on_its_instance(insp, random_plan, nan_word, place_words, nodes_word):
    """one NaN state entry (instance 1, node 2): that instance's record says so (word nan_word NaN, its place_words -1, nodes_word
    N), the other instances keep their bits, and the nodes behind node 2 do not see it"""
    model, N, B = "srbd13", 6, 3
    batch, x, u, P = random_plan(model, N, B, seed=5)
    eng = engine_with_plan(model, N, B, batch["consts"], P, batch)
    clean = run(insp, eng, x=x, u=u)
    bad = x.copy()
    bad[1, 2, 4] = np.nan                                                       # instance 1, node 2, one state (quaternion) entry
    got = run(insp, eng, x=bad, u=u)
    assert np.isnan(got[0][1, nan_word]) and all(got[0][1, w] == -1 for w in place_words)
    assert got[0][1, nodes_word] == N
    keep = [0, 2]
    assert all(a[keep].tobytes() == b_[keep].tobytes() for a, b_ in zip(got, clean))
    assert np.isnan(got[1][1, 2]).any() and not np.isnan(got[1][1, 3:]).any()    # the nodes behind it do not see node 2
    eng.close()


def touch_with(insp, **sub):
    """the `touch` of assert_nothing_else_moves for an inspector: the host twin, the handle's own plan whole and in a sub-range (with
    `sub`) and the warm start as a caller's trajectory -> every result's bytes"""
    def touch(eng, batch, x):
        got = (insp.host(eng), *insp.device(eng), *insp.device(eng, 1, 3, **sub), *insp.device(eng, x=batch["xs"], u=batch["us"]))
        return tuple(a.tobytes() for a in got)
    return touch


def assert_nothing_else_moves(touch, opts, policy=False):
    """touch(eng, batch, x) -> bytes makes the calls under test on a handle that has solved `batch` to the plan x (srbd13, N = 6, 5
    instances; eng.knots = 4 kept knots where the handle has a policy, else 0).  Nothing of the handle but the calls' own outputs may
    move.  policy: the calls need a policy, so every handle here exports one; else only the first does."""
    model, N, B, M = "srbd13", 6, 5, 4
    batch = workload.make_batch(model, N, np.arange(B) + 3)

    def handle(with_policy=policy, resume=False, log=False, auto=False, **over):
        eng = DdpEngine(model, N, B, opts=dict(opts, **over), consts=batch["consts"])
        if resume:
            eng.enable_resume()
        if log:
            eng.enable_iteration_log(8)
        if auto:
            eng.enable_auto_classes()
        eng.knots = M if with_policy else 0      # (for run and for touch)
        if with_policy:
            eng.enable_policy(M)
        return eng

    def run(eng):
        out = solve(eng, batch)
        if eng.knots:
            eng.policy_range_device()
        return out

    def forward_after_backward(eng, x):      # the slots' work buffers: a forward after a backward, with and without the calls between them
        eng.backward(batch["params"], 1e-6)
        ref = eng.forward(batch["params"], 0.5)
        eng.backward(batch["params"], 1e-6)
        touch(eng, batch, x)
        assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(eng.forward(batch["params"], 0.5), ref))

    # a cut solve with everything a handle can carry: plan, stats, policy, resume flags, iteration log, what the last launch left
    eng = handle(True, resume=True, log=True, max_iters=2)
    x, u, st = run(eng)
    assert eng.unfinished() > 0                                                      # there are resume flags to keep

    def state():
        xs, us, stats = eng.fetch()
        for f in st.dtype.names:
            np.testing.assert_array_equal(stats[f], st[f], err_msg=f)
        rec, n = eng.iteration_log()
        return (xs.tobytes(), us.tobytes(), stats.tobytes(), eng.fetch_policy().tobytes(), eng.unfinished(), eng.unfinished(1, 3),
                rec.tobytes(), n.tobytes(), eng.queue_info(), eng.kernel_info())

    before = state()
    assert before[:2] == (x.tobytes(), u.tobytes())
    touch(eng, batch, x)
    assert state() == before
    forward_after_backward(eng, x)
    eng.close()
    # the class labels and their history of a handle that labels its instances itself; and an ordinary handle's work buffers
    eng = handle(auto=True, queue_order=3)
    x = run(eng)[0]
    labels = lambda: (eng._host_copy(_lib.BUF_CLASSES, "<i4").tobytes(), eng.auto_classes_info())      # noqa: E731
    before = labels()
    touch(eng, batch, x)
    assert labels() == before
    forward_after_backward(eng, x)
    eng.close()
    # a cut solve continued after the calls is the one continued without them
    ends = []
    for call in (False, True):
        eng = handle(resume=True, max_iters=2)
        x = run(eng)[0]
        if call:
            touch(eng, batch, x)
        eng.set_options(max_iters=100)
        eng.continue_solve()
        ends.append(tuple(a.tobytes() for a in eng.fetch()))
        eng.close()
    assert ends[0] == ends[1]
    # a solve after the calls is the solve of a fresh handle; two slots for five instances, so the queue and the slots' buffers are in play
    used, fresh = handle(max_slots=2), handle(max_slots=2)
    assert used.queue_info()[0] == 2
    touch(used, batch, run(used)[0])
    after, ref = run(used), run(fresh)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(after, ref))
    assert touch(used, batch, after[0]) == touch(fresh, batch, ref[0])
    used.close()
    fresh.close()


def assert_common_refusals(insp, opts):
    """what every inspector refuses, in the words all of them use, and that the handle works afterwards"""
    model, N, B = "srbd13", 6, 2
    batch = workload.make_batch(model, N, [0, 1])
    eng = DdpEngine(model, N, B, opts=opts)
    for call in (lambda: insp.host(eng), lambda: insp.device(eng)):
        with pytest.raises(RuntimeError, match="no solve has run"):
            call()
    x, u, _ = solve(eng, batch)
    gx, gu, out = dev(x), dev(u), torch.zeros((B, insp.words), dtype=torch.float64, device="cuda")
    vp = lambda t: eng._dev(t, t.shape)      # noqa: E731
    for dx, du in ((vp(gx), None), (None, vp(gu))):                                 # one of d_x / d_u NULL
        with pytest.raises(RuntimeError, match="both NULL"):
            eng._chk(insp.raw(eng, 0, B, dx, du, vp(out)))
    with pytest.raises(RuntimeError, match="NULL argument"):
        eng._chk(insp.raw(eng, 0, B, None, None, None))
    for call in (lambda: insp.device(eng, 1, 2), lambda: insp.host(eng, 1, 2), lambda: insp.host(eng, -1, 1), lambda: insp.host(eng, 0, 0)):
        with pytest.raises(RuntimeError, match="range outside"):
            call()
    assert insp.raw(eng, 1, 2, None, None, vp(out)) == -1                           # SDDP_ERR_ARG
    assert insp.host(eng).shape == (B, insp.words)                                  # and the handle still works
    eng.close()
    return batch, x, u


def assert_fleet_queue_follows_the_last_flush(insp, opts, optional=None):
    """FleetQueue.<name> (the audit: flush(audit_out=)) covers what the last flush solved: 0 and nothing launched before any, a partial
    handle, a full handle with the optional output `optional`, a guard row of 7.0 behind them -> (eng, batch, the full handle's records)"""
    model, N, batch_n, depth = "srbd13", 6, 4, 2
    batch = workload.make_batch(model, N, np.arange(batch_n) + 3)
    eng = DdpEngine(model, N, batch_n * depth, opts=opts, consts=batch["consts"])
    t = {k: dev(batch[k]) for k in ("x0", "xs", "us", "params")}
    fleet = FleetQueue(eng, t["params"].repeat(depth, 1, 1).contiguous(), batch_n, depth)
    out = torch.full((batch_n * depth + 1, insp.words), 7.0, dtype=torch.float64, device="cuda")

    def flush_and_inspect(**opt):
        if insp is AUDIT:
            return fleet.flush(audit_out=out)
        return min(fleet.flush(), getattr(fleet, insp.name)(out, **opt))

    if insp is not AUDIT:
        assert getattr(fleet, insp.name)(out) == 0                                  # nothing flushed yet: nothing launched
        assert np.all(out.cpu().numpy() == 7.0)
    fleet.submit(t["x0"], t["xs"], t["us"])
    assert flush_and_inspect() == batch_n                                           # a partial handle: the first block alone
    eng.synchronize()
    got = out.cpu().numpy()
    assert got[:batch_n].tobytes() == insp.host(eng, 0, batch_n).tobytes() and np.all(got[batch_n:] == 7.0)
    fleet.submit(t["x0"], t["xs"], t["us"])
    fleet.submit(t["x0"], t["xs"], t["us"])
    opt = {} if optional is None else {optional: torch.full((batch_n * depth, *insp.optional[optional](eng)), 7.0, dtype=torch.float64, device="cuda")}
    assert flush_and_inspect(**opt) == batch_n * depth
    eng.synchronize()
    got = out.cpu().numpy()
    ref = insp.device(eng)
    assert got[:-1].tobytes() == ref[0].tobytes() == insp.host(eng).tobytes() and np.all(got[-1] == 7.0)
    if optional is not None:
        assert opt[optional].cpu().numpy().tobytes() == ref[1 + list(insp.optional).index(optional)].tobytes()
    assert got[:batch_n].tobytes() == got[batch_n:2 * batch_n].tobytes()            # the same robots in both blocks
    return eng, batch, got[:-1]


# ---- another iteration count than the oracle ---------------------------------------------------------------------------------------------
def explain(c, s, opts, engine_over, idx, cst=None):
    """the instances on another iteration count than the oracle: one-step shadowing of the GPU path (tests/shadow.py).  cst: the
    oracle's constants where they are not RobotConsts(**s["consts"]) (srbd61 with other feet: tests/consts_cases.py oracle_consts)"""
    from tests import shadow
    recs = shadow.explain_divergent(c.model, c.N, opts, engine_over, s["consts"], omodels.RobotConsts(**s["consts"]) if cst is None else cst, s, idx)
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
