"""The references under the case tables, each written once: the frozen workload batch, the C oracle on a start (a batch, or one
instance with its line-search trace), the optimum under BASE that serves as a restart point, and the option dictionary of a case.
numpy and the oracle only, no GPU: CPU tests import this module.  Plain functions, no fixtures.  A start is a dict(x0, params, xs,
us, consts); the case modules (tests/*_cases.py) keep the tables, the measured figures and the caches by case name.  The names of the
stats columns belong to their producer: cport.STAT_FIELDS, read with cport.stat."""
import functools

import numpy as np

from oracle import cport, ddp as oddp, models as omodels
from srbd_horizon_amd import workload

BASE = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)      # dsrbd_example.py:55-58
ARRAYS = ("x0", "params", "xs", "us")


def frozen(arrays):
    """a cached reference, read-only: one array, a sequence of arrays, or a start (its x0, params, xs, us) -> the same object"""
    each = (arrays,) if isinstance(arrays, np.ndarray) else [arrays[k] for k in ARRAYS] if isinstance(arrays, dict) else arrays
    for a in each:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _batch(model, N, seeds):
    return frozen(workload.make_batch(model, N, list(seeds)))


def batch(model, N, seeds):
    """workload.make_batch(model, N, seeds), made once: x0, params, xs, us read-only -> a dict of the caller's own"""
    return dict(_batch(model, int(N), tuple(int(s) for s in seeds)))


def options(over, **more):
    """BASE with the override dictionary `over`, then `more`: the options of both sides, DdpEngine(opts=...) and oddp.DdpOptions(**...)"""
    return {**BASE, **over, **more}


def case_options(case, **more):
    """the option dictionary of a case: options(case.over, **more)"""
    return options(case.over, **more)


def consts(start):
    """the oracle's constants of a start: RobotConsts(**start["consts"])"""
    return omodels.RobotConsts(**start["consts"])


def _args(start, opts, cst, sel, replace):
    """what cport.solve_batch / solve_trace take first: constants, options and the four arrays of the instances `sel`"""
    s = dict(start, **replace)
    return (consts(start) if cst is None else cst, oddp.DdpOptions(**opts), *(np.asarray(s[k])[sel] for k in ARRAYS))


def c_oracle(model, start, opts, variant="off", *, cst=None, sel=slice(None), threads=4, **replace):
    """-> (xs [B,N+1,nx], us [B,N,nu], stats [B,8]: cport.STAT_FIELDS) of the C oracle build `variant` on the start, read-only.
    cst: a RobotConsts other than RobotConsts(**start["consts"]); sel: the instances to solve (a slice, indices); replace: arrays in
    place of the start's (xs=..., params=...)"""
    with np.errstate(all="ignore"):
        return frozen(cport.solve_batch(*_args(start, opts, cst, sel, replace), threads=threads, model=model, variant=variant))


def c_trace(model, start, opts, b, variant="off", *, cst=None, cap=256, resume=None, **replace):
    """-> (xs, us, stats [8], line-search records) of cport.solve_trace on instance b of the start; cap, resume: solve_trace's"""
    return cport.solve_trace(*_args(start, opts, cst, b, replace), model=model, variant=variant, cap=cap, resume=resume)


@functools.lru_cache(maxsize=None)
def optimum(model, N, seeds):
    """-> (xs, us) the C oracle (`off`) reaches under BASE from the workload's warm start, every instance converged: a restart point"""
    xs, us, st = c_oracle(model, batch(model, N, seeds), BASE)
    assert (cport.stat(st, "converged") == 1).all() and (cport.stat(st, "status") == 0).all(), (model, N, seeds, st)
    return xs, us
