"""ms per MPC tick at B = 1 (srbd13, N = 30): the loop of bench.py single_instance_extras (mpc.MpcLoop, walking forward, 20 warm-up +
200 timed ticks), without the CPU baselines of --full.  One JSON line."""
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from srbd_horizon_amd.mpc import MpcLoop  # noqa: E402

gc.collect(); gc.freeze()
loop = MpcLoop("srbd13", 30, warm_start="device")
ms = []
for i in range(220):
    t1 = time.perf_counter()
    loop.tick("walking", (1.0, 0.0))
    ms.append(1e3 * (time.perf_counter() - t1))
ms = np.array(ms[20:])
print(json.dumps({"tree": sys.argv[1], "ms_per_mpc_tick_median": float(np.median(ms)), "p10": float(np.percentile(ms, 10)),
                  "p90": float(np.percentile(ms, 90)), "p99": float(np.percentile(ms, 99)), "solve_median": float(np.median(loop.solve_ms[20:]))}))
