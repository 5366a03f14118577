"""Price of the per-instance constants table on identical work: the SAME handle solves the same cold batch without the table and
with a table whose rows all repeat the handle's constants (bit-identical results), so the time ratio is the row fetch plus any
difference in register allocation of the `_h` kernels.  Kernel time by HIP events on the handle's stream (it covers the
queue_order 2 key pre-pass and the sort), 2 warm-up + 7 timed launches per mode, modes alternating.  One JSON line per case:

    python profiles/hetero/hetero_cost.py >> profiles/hetero/hetero_cost.jsonl
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from srbd_horizon_amd import workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402

OPTS = dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3, queue_order=2)
CASES = [("srbd13", 30, 20480, 2), ("srbd37", 20, 2048, 2), ("srbd37", 20, 2048, 1)]
WARM, TIMED = 2, 7


def launch_ms(e, b):
    e.set_initial_state(b["x0"]); e.set_x_warmstart(b["xs"]); e.set_u_warmstart(b["us"]); e.synchronize()
    e.kernel_time_stats(reset=True)
    e.solve_resident()
    ms, n = e.kernel_time_stats(reset=True)
    assert n == 1
    return ms


def main():
    for model, N, B, wps in CASES:
        b = workload.make_batch(model, N, np.arange(B))
        e = DdpEngine(model, N, B, opts=dict(OPTS, waves_per_simd=wps), consts=b["consts"])
        e.enable_timing(True)
        e.set_params(b["params"])
        ms = {"homogeneous": [], "table": []}
        info, ref = {}, None
        for rep in range(WARM + TIMED):
            for mode in ("homogeneous", "table"):
                if mode == "table":
                    e.set_instance_consts({"m": np.full(B, e.consts.m)})
                else:
                    e.clear_instance_consts()
                t = launch_ms(e, b)
                if rep >= WARM:
                    ms[mode].append(t)
                info[mode] = e.kernel_info().get("resources")
                x, u, st = e.fetch()
                if ref is None:
                    ref = (x.copy(), u.copy(), st.tobytes())
                assert np.array_equal(x, ref[0]) and np.array_equal(u, ref[1]) and st.tobytes() == ref[2]
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(json.dumps(dict(model=model, N=N, batch=B, waves_per_simd=wps, queue_order=2, warmup=WARM, timed=TIMED, kernel_ms=ms,
                              median_ms=med, ratio_table_over_homogeneous=med["table"] / med["homogeneous"],
                              solves_per_s={k: B / (v * 1e-3) for k, v in med.items()}, resources=info,
                              mean_iters=float(e.stats["iters"].mean()), bit_identical=True)), flush=True)
        e.close()


if __name__ == "__main__":
    main()
