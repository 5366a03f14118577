"""Host path of one B = 1 tick (sddp_advance + sddp_solve_resident), median over many ticks; library chosen by SDDP_LIB."""
import gc, sys, time
import numpy as np
sys.path.insert(0, ".")
from srbd_horizon_amd import workload
from srbd_horizon_amd.engine import DdpEngine
N = 30
b = workload.make_batch("srbd13", N, [0])
e = DdpEngine("srbd13", N, 1, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3))
e.set_initial_state(b["x0"]); e.set_x_warmstart(b["xs"]); e.set_u_warmstart(b["us"]); e.set_params(b["params"])
x, u = e.solve_resident()
p_last = b["params"][:, -1].copy()
gc.collect(); gc.freeze()
t = []
for i in range(4000):
    x0 = x[:, 1].copy()
    t0 = time.perf_counter()
    e.advance(p_last, x0)
    x, u = e.solve_resident()
    t.append(1e6 * (time.perf_counter() - t0))
t = np.array(t[500:])
print(f"{sys.argv[1]} tick_us median {np.median(t):.2f} p10 {np.percentile(t, 10):.2f} p90 {np.percentile(t, 90):.2f} iters {int(e.stats['iters'][0])}")
