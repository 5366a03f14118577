#!/usr/bin/env python3
"""Auto classes (sddp_enable_auto_classes): what the label kernel adds to a queue_order = 3 launch at the bench shape.

    python profiles/auto_classes/measure.py --labels host [--launches 5]     one JSON line; with SDDP_LIB pointing at the parent's
                                                                             library: (a), at this tree's: (b)
    python profiles/auto_classes/measure.py --labels auto [--launches 5]     one JSON line: (c)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/auto_classes/measure.py --labels auto
    python profiles/auto_classes/measure.py --digest DIR                     the kernels' rows of DIR's *kernel_stats.csv

Shape: srbd13, N = 30, 20 480 instances (the 1024 bench instances, workload.make_batch seeds 0..1023, 20 times over) in ONE launch,
waves_per_simd = 2, queue_order = 3.  host: the labels are workload.srbd13_schedule_classes, uploaded with
sddp_set_instance_classes before the first launch (what bench.py does); auto: sddp_enable_auto_classes and no label ever passed.
Every launch runs on the batch reloaded before it; the time is the HIP-event interval of the launch sequence
(sddp_enable_timing / sddp_last_kernel_ms): key pre-pass, sort, solve kernel, class update -- and the label kernel under auto.
One warm-up launch (no history yet: initial-cost order) comes first and is not reported."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from srbd_horizon_amd import _lib, workload  # noqa: E402

NEW = ("sddp_enable_auto_classes", "sddp_auto_classes_info", "sddp_fetch_instance_classes", "sddp_get_class_stats", "sddp_add_class_stats")
OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3, waves_per_simd=2, queue_order=3)
MODEL, N, SEEDS, TIMES = "srbd13", 30, 1024, 20


def digest(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    for path in files:
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            print(json.dumps({"kernel": name[:100], "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", choices=("host", "auto"))
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--digest")
    args = ap.parse_args()
    if args.digest:
        return digest(args.digest)
    import ctypes
    import torch  # noqa: F401  (its HIP runtime first, as _lib.load does)
    if not hasattr(ctypes.CDLL(_lib.LIB_PATH), NEW[0]):          # a parent library: (a)
        if args.labels == "auto":
            raise SystemExit("this library has no auto classes")
        for name in NEW:
            _lib.SYMBOLS.pop(name)
    from srbd_horizon_amd.engine import DdpEngine
    b = workload.make_batch(MODEL, N, np.arange(SEEDS))
    t = {k: np.ascontiguousarray(np.concatenate([b[k]] * TIMES)) for k in ("x0", "xs", "us", "params")}
    eng = DdpEngine(MODEL, N, SEEDS * TIMES, opts=OPTS, consts=b["consts"])
    if args.labels == "host":
        eng.set_instance_classes(*workload.srbd13_schedule_classes(t["params"]))
    else:
        eng.enable_auto_classes()
    eng.enable_timing()
    eng.set_params(t["params"])

    def launch():
        eng.set_initial_state(t["x0"]); eng.set_x_warmstart(t["xs"]); eng.set_u_warmstart(t["us"])
        eng.solve_resident_first()
        eng.synchronize()
        return eng.last_kernel_ms()

    launch()
    ms = [round(launch(), 4) for _ in range(args.launches)]
    out = {"lib": os.path.relpath(_lib.LIB_PATH, _lib.ROOT), "labels": args.labels, "model": MODEL, "N": N, "instances": SEEDS * TIMES,
           "queue": list(eng.queue_info()), "iters_sum": int(eng.first_stats["iters"].sum()), "launch_ms": ms}
    if args.labels == "auto":
        out["labels_equal_host"] = bool(np.array_equal(eng.instance_classes(), workload.srbd13_schedule_classes(t["params"])[0]))
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
