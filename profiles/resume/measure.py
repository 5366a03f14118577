#!/usr/bin/env python3
"""What resumable solves cost and buy on a cold 1024-robot srbd13 tick (N = 30, the bench instances: workload.make_batch seeds 0..1023).

    python profiles/resume/measure.py [--reps 7] [--resources]

Prints one JSON line.  Times are host wall-clock medians over `--reps` repetitions of: load the batch, launch, wait.
  uncut_ms            ordinary handle, one launch at max_iters = 100, records packed behind it
  resumable_uncut_ms  the same launch on a handle with sddp_enable_resume (the overhead: flag and, for status 1, the dft store at exit)
  first_records_ms    sliced: launch at max_iters = 6 + first-knot records + the unfinished count on the host
  last_record_ms      sliced: the above + the continue launch + records
--replay: the 1024-robot srbd13 fleet tick of bench.py's fleet_tick instead (waves_per_simd = 1, N = 30: one cold solve of the bench
  instances, then 100 warm ticks, each robot where its plan said, warm-started from its previous solution advanced by one knot by
  sddp_advance; the first 4 ticks dropped), closed through the first-knot records like fleet_tick's run_first.  Per tick:
    uncut      sddp_advance + sddp_solve_resident_first at max_iters = 100 (ordinary handle; `resumable`: the same with sddp_enable_resume)
    sliced     sddp_advance + sddp_solve_resident_first at max_iters = 6 -> the first records are on the host (first_ms); if a robot is
               unfinished: max_iters = 100, sddp_continue_resident, first-knot records packed and copied (last_ms)
  The sliced loop visits the same states as the uncut one (checked: `identical`), so all three replay the same trace.
--resources: sddp_kernel_resources of every plain build, ordinary and resumable."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from srbd_horizon_amd import workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402
from srbd_horizon_amd.fleet import FleetQueue  # noqa: E402

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3)


def resources():
    out = {}
    for model, N in (("srbd13", 30), ("srbd37", 20), ("lip30", 20), ("srbd61", 20)):
        b = workload.make_batch(model, N, [0, 1])
        for wps in (1, 2):
            for res in (False, True):
                eng = DdpEngine(model, N, 2, opts=dict(OPTS, waves_per_simd=wps, max_iters=2), consts=b["consts"])
                if res:
                    if not hasattr(eng, "enable_resume"):
                        continue
                    eng.enable_resume()
                eng.set_initial_state(b["x0"]); eng.set_x_warmstart(b["xs"]); eng.set_u_warmstart(b["us"])
                eng.solve(b["params"])
                info = eng.kernel_info()
                out[f"{info['kernel']}{' resumable' if res else ''} (asked w{wps})"] = info["resources"]
                eng.close()
    return out


def replay(R, k, ticks=100, total=100):
    N = 30
    b = workload.make_batch("srbd13", N, np.arange(R))
    p_last = b["params"][:, -1].copy()                       # the plan's last column repeats
    dev = torch.device("cuda", 0)

    def run(resume, sliced):
        e = DdpEngine("srbd13", N, R, opts=dict(OPTS, waves_per_simd=1), consts=b["consts"])
        if resume:
            e.enable_resume()
        nu, nx = e.nu, e.nx
        rec = torch.empty((R, e.record_words("first_knot")), dtype=torch.float64, device=dev)
        e.set_initial_state(b["x0"]); e.set_x_warmstart(b["xs"]); e.set_u_warmstart(b["us"])
        e.set_params(b["params"])
        u0, x1 = e.solve_resident_first()
        first, last, unfin, states = [], [], [], []
        for t in range(ticks):
            t0 = time.perf_counter()
            if sliced:
                e.set_options(max_iters=k)
            e.advance(p_last, x1)
            u0, x1 = e.solve_resident_first()
            t1 = t2 = time.perf_counter()
            n = int((e.first_stats["status"] == 1).sum()) if sliced else 0
            if n:
                e.set_options(max_iters=total)
                e.continue_solve()
                e.pack_records_device(rec, 0, R, "first_knot")
                e.synchronize()
                h = rec.cpu().numpy()
                u0, x1 = h[:, :nu].copy(), h[:, nu:nu + nx].copy()
                t2 = time.perf_counter()
            first.append(1e3 * (t1 - t0)); last.append(1e3 * (t2 - t0)); unfin.append(n); states.append(x1.copy())
        e.close()
        return np.array(first[4:]), np.array(last[4:]), np.array(unfin[4:]), np.array(states)

    q = lambda a: dict(median=round(float(np.median(a)), 3), p99=round(float(np.percentile(a, 99)), 3), max=round(float(a.max()), 3))
    _, lu, _, su = run(False, False)
    _, lr, _, sr = run(True, False)
    fs, ls, un, ss = run(True, True)
    return {"replay": {"robots": R, "ticks": int(len(lu)), "first_slice": k, "uncut_ms": q(lu), "resumable_uncut_ms": q(lr),
                       "sliced_first_ms": q(fs), "sliced_last_ms": q(ls),
                       "fraction_finished_after_first_slice": round(float(1.0 - un.mean() / R), 5),
                       "ticks_with_a_second_launch": int((un > 0).sum()), "unfinished_per_tick_max": int(un.max()),
                       "identical": bool(su.tobytes() == sr.tobytes() == ss.tobytes())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--first-slice", type=int, default=6)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--replay", action="store_true")
    args = ap.parse_args()
    if args.replay:
        print(json.dumps(replay(args.robots, args.first_slice)))
        return
    if args.resources:
        print(json.dumps({"resources": resources()}))
        return
    R, N, k = args.robots, 30, args.first_slice
    dev = torch.device("cuda", 0)
    b = workload.make_batch("srbd13", N, np.arange(R))
    d = {n: torch.from_numpy(b[n]).to(dev) for n in ("x0", "xs", "us", "params")}
    out = {"robots": R, "first_slice": k}

    def run(resume, sliced):
        eng = DdpEngine("srbd13", N, R, opts=dict(OPTS, waves_per_simd=2), consts=b["consts"])
        if resume:
            eng.enable_resume()
        fleet = FleetQueue(eng, d["params"], R, 1)
        rec = torch.empty((R, eng.record_words("first_knot")), dtype=torch.float64, device=dev)
        t_first, t_last, fin = [], [], 0
        for rep in range(args.reps + 2):
            fleet.submit(d["x0"], d["xs"], d["us"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if not sliced:
                fleet.flush()
                eng.pack_records_device(rec, 0, R, "first_knot")
                torch.cuda.synchronize()
                t1 = t2 = time.perf_counter()
            else:
                eng.set_options(max_iters=k)
                eng.solve_range_device(d["params"], 0, R)
                eng.pack_records_device(rec, 0, R, "first_knot")
                n = eng.unfinished()                             # waits for the stream: the first records are there
                t1 = time.perf_counter()
                eng.set_options(max_iters=100)
                if n:
                    eng.continue_solve(d["params"])
                    eng.pack_records_device(rec, 0, R, "first_knot")
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                fleet.pending = 0
                fin = R - n
            if rep >= 2:
                t_first.append(1e3 * (t1 - t0)); t_last.append(1e3 * (t2 - t0))
        st = eng.fetch()[2]
        eng.close()
        return statistics.median(t_first), statistics.median(t_last), fin, st

    u1, _, _, st_u = run(False, False)
    r1, _, _, st_r = run(True, False)
    f1, l1, fin, st_s = run(True, True)
    out.update(uncut_ms=round(u1, 3), resumable_uncut_ms=round(r1, 3), first_records_ms=round(f1, 3), last_record_ms=round(l1, 3),
               finished_after_first_slice=fin, fraction_finished=round(fin / R, 4), iters_mean=float(st_u["iters"].mean()),
               iters_max=int(st_u["iters"].max()),
               identical=bool(st_u.tobytes() == st_r.tobytes() == st_s.tobytes()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
