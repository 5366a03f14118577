"""What every instance did on its way through a solve: the iteration log (include/sddp.h, sddp_enable_iteration_log).

    python examples/iteration_log.py

Solves the 48 srbd13 instances of tests/resume_cases.py at N = 30, prints the line searches of the three longest solves (step
length, cost, expected against actual reduction, regularisation, second-order switch, candidates tried) and a histogram of the
accepted step lengths over all instances."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srbd_horizon_amd import _lib, workload  # noqa: E402
from srbd_horizon_amd.engine import DdpEngine  # noqa: E402

N, B, ROWS = 30, 48, 128
F = {n: i for i, n in enumerate(_lib.LOG_FIELDS)}


def main():
    b = workload.make_batch("srbd13", N, list(range(B)))
    eng = DdpEngine("srbd13", N, B, opts=dict(max_iters=100, alpha_converge_threshold=1e-12, beta=1e-3), consts=b["consts"])
    eng.enable_resume()                      # the log is kept by the resumable kernels
    eng.enable_iteration_log(ROWS)
    eng.load(b["x0"], b["xs"], b["us"])
    eng.solve(b["params"])
    st = eng.stats.copy()
    rec, n = eng.iteration_log()
    eng.close()
    for i in np.argsort(-st["iters"], kind="stable")[:3]:
        print(f"instance {i}: {st['iters'][i]} iterations, {n[i]} line searches, {st['rollouts'][i]} rollouts, status {st['status'][i]}")
        print(f"  {'#':>3} {'alpha':>10} {'J':>14} {'expected':>11} {'actual':>11} {'mu':>9} {'theta':>5} {'tried':>5} {'bumps':>5}")
        for j, r in enumerate(rec[i, :n[i]]):
            actual = r[F["J"]] - r[F["J_accepted"]] if r[F["alpha"]] > 0.0 else float("nan")
            print(f"  {j:>3} {r[F['alpha']]:>10.3g} {r[F['J']]:>14.6f} {r[F['expected']]:>11.3e} {actual:>11.3e} {r[F['mu']]:>9.2e} "
                  f"{int(r[F['theta']]):>5} {int(r[F['tried']]):>5} {int(r[F['mu_bumps']]):>5}")
    hist = collections.Counter()
    for i in range(B):
        hist.update(rec[i, :n[i], F["alpha"]].tolist())
    total = sum(hist.values())
    print(f"accepted step lengths over {total} line searches of {B} instances (0: the search failed):")
    for a in sorted(hist, reverse=True):
        print(f"  {a:>10.3g} {hist[a]:>5} {'#' * max(1, round(60 * hist[a] / total))}")


if __name__ == "__main__":
    main()
