"""A fleet of independent MPC instances fed to ONE engine handle as a work queue ("work queue").

The engine holds ``depth`` batches of ``batch`` instances each.  ``submit`` loads one batch (initial state, warm start and,
optionally, its parameters) into the next free block of the handle; ``flush`` solves everything submitted since the last
flush in ONE launch: the resident workgroups of the device pull instances from a queue until it is empty, so the slowest
instances overlap with all the others instead of ending a launch alone (one batch = 1024 instances never fills the 2048
resident wavefronts of an MI355X, and a launch lasts as long as its slowest instance).

With more than one rank (instances sharded contiguously across the GPUs of a node) a flush closes with
the one collective of the path, an all-gather of the solution records of the solved blocks (RCCL over xGMI on GPUs, gloo in the
CPU test).  The collective is ASYNCHRONOUS and double buffered: the records of launch k are packed into pack buffer k mod 2
on the engine's stream (behind the solve), ``all_gather_into_tensor(async_op=True)`` fills gather buffer k mod 2, and the next
batches are loaded and launch k + 1 starts while it is on the wire.  A buffer pair is waited for before it is reused (at
flush k + 2) and by ``wait()`` -- which the caller runs before reading ``gathered`` and at the end of a timed region.  All
buffers are allocated once, in ``__init__`` (``depth * batch`` records per rank), never per flush.

``submit`` raises when the handle is full: the results of the pending batches live in the handle's buffers and the next load
would overwrite them, so the caller decides when to launch and when the results have been consumed (``flush`` / ``wait``).

This is the step function of ``bench.py``; ``tests/test_fleet_gloo.py`` drives the same class at world size 2 on CPU with an
engine stand-in.  The engine only needs ``load_range_device``, ``solve_range_device`` and ``fetch_device_views`` (with
``policy=True`` also ``policy_range_device`` and, for a stand-in, a ``policy_records`` tensor [B, words]) (and, on a
GPU, ``use_torch_stream``: packing and the collective are torch operations on torch's current stream, so the engine is bound to
that stream here).
"""
from __future__ import annotations

from . import _lib
from . import dist as sdist


class FleetQueue:
    def __init__(self, engine, params_all, batch: int, depth: int, collective: bool = False, gather: str = "full",
                 policy: bool = False):
        """gather: what the closing all-gather carries per instance -- "full": x | u | cost | iterations, the whole plan
        (4 680 B at (30, 13, 6)); "first_knot": u_0 | x_1 | cost | iterations (168 B), what a fleet in
        closed loop needs from the other ranks.
        policy: every flush runs the policy launch behind the solve (the engine's enable_policy must have been called) and the
        first-knot record carries the first knot's gains behind it: u_0 | x_1 | cost | iterations | kff_0 | K_0."""
        self.eng, self.P, self.batch, self.depth, self.collective = engine, params_all, int(batch), int(depth), bool(collective)
        if gather not in ("full", "first_knot"):
            raise ValueError("gather must be 'full' or 'first_knot'")
        if policy and gather != "first_knot":
            raise ValueError("policy=True extends the 'first_knot' record")
        self.policy = bool(policy)
        self.gather = "first_knot_policy" if policy else gather
        if tuple(params_all.shape[:1]) != (self.batch * self.depth,):
            raise ValueError("params_all must hold depth * batch instances")
        self.pending = 0            # batches loaded and not yet solved
        self.solved = 0             # instances [0, solved) of the handle: what the most recent solving call covered
        self.launches = 0
        self.gather_bytes = 0       # bytes this rank contributed to the collectives so far
        self.x, self.u, self.sf, self.si = engine.fetch_device_views()
        if self.x.is_cuda:
            import torch
            # solve, pack and collective must be ordered on ONE stream: torch's current one
            engine.use_torch_stream(torch.cuda.current_stream())
        self._work = [None, None]   # outstanding collective per buffer pair
        self._n = [0, 0]            # instances per rank in that collective
        self._k = 0                 # buffer pair of the next flush
        self._last = None           # buffer pair of the most recent flush
        self._pack = self._out = None
        if self.collective:
            import torch
            import torch.distributed as dist
            self.world = dist.get_world_size()
            words = sdist.record_words(self.x.shape[1] - 1, self.x.shape[2], self.u.shape[2], self.gather)
            cap = self.batch * self.depth
            mk = lambda rows: torch.empty((rows, words), dtype=torch.float64, device=self.x.device)
            self._pack = [mk(cap), mk(cap)]
            self._out = [mk(self.world * cap), mk(self.world * cap)]

    @property
    def full(self) -> bool:
        return self.pending == self.depth

    def submit(self, x0, xs, us, params=None, classes=None, n_classes=0):
        """One step: one batch of instances enters the queue (device tensors of `batch` instances; `params` [batch, N+1, np]
        replaces that block's parameters; `classes` [batch] int32 labels them for queue_order 3, sddp.h).  On an engine with
        enable_auto_classes() pass no `classes`: the flush's launch labels every instance it solves itself, from `params_all` as it
        stands then (labels passed to such an engine raise).  Raises when the handle is full: flush first."""
        if self.pending == self.depth:
            raise RuntimeError("FleetQueue is full: flush() (and consume the results) before submitting another batch")
        lo = self.pending * self.batch
        if params is not None:
            self.P[lo:lo + self.batch].copy_(params)
        if classes is not None:
            self.eng.set_instance_classes_range_device(lo, self.batch, classes, n_classes)
        self.eng.load_range_device(lo, self.batch, x0, xs, us)
        self.pending += 1

    def set_instance_consts(self, overrides: dict, first: int = 0):
        """Per-instance robot constants of this shard's handle (DdpEngine.set_instance_consts): `first` counts within the handle,
        i.e. instance `first` of block 0 is the first instance of the first submitted batch.  Ordered on the engine's stream, so
        it may be called between a flush and the next submit."""
        self.eng.set_instance_consts(overrides, first)

    def clear_instance_consts(self):
        self.eng.clear_instance_consts()

    def flush(self, audit_out=None):
        """Solve the pending batches in one launch (asynchronous); with a process group, start the all-gather of their solution
        records (asynchronous too: `wait()` before reading `gathered`).
        audit_out: a device tensor [>= n, AUDIT_WORDS]; the plan audit of the solved instances (DdpEngine.audit_device) is launched
        behind the solve and the policy launch into its first n rows."""
        n = self.pending * self.batch
        if n == 0:
            return 0
        self.eng.solve_range_device(self.P, 0, n)
        if self.policy:
            self.eng.policy_range_device(0, n)                               # one sweep per instance at the returned iterate
        self.solved = n
        if audit_out is not None:
            self._inspect(self.eng.audit_device, audit_out)
        self.launches += 1
        if self.collective:
            import torch.distributed as dist
            k = self._k
            self._wait(k)                                                    # this pair's previous collective (two flushes ago)
            if hasattr(self.eng, "pack_records_device"):                   # the HIP engine: ONE kernel behind the solve
                local = self.eng.pack_records_device(self._pack[k][:n], 0, n, self.gather)
            else:                                                            # engine stand-in of the CPU tests
                local = sdist.pack_records_into(self._pack[k][:n], self.x[:n], self.u[:n], self.sf[:n, _lib.STATS_F64_COST],
                                                self.si[:n, _lib.STATS_I32_ITERS], self.gather,
                                                self.eng.policy_records[:n] if self.policy else None)
            self._work[k] = dist.all_gather_into_tensor(self._out[k][:self.world * n], local, async_op=True)
            self._n[k] = n
            self.gather_bytes += local.numel() * local.element_size()
            self._last = k
            self._k ^= 1
        self.pending = 0
        return n

    def _inspect(self, launch, out, **optional):
        """launch (an inspector's *_device method of the engine) on the instances the most recent solving call covered, into the
        first n rows of out and of every optional output that is not None -> n; 0, and nothing launched, before the first such call"""
        n = self.solved
        if n:
            launch(out[:n], 0, n, **{k: None if t is None else t[:n] for k, t in optional.items()})
        return n

    def stationarity(self, out, lam=None, grad=None):
        """The stationarity records (DdpEngine.stationarity_device) of the instances the last flush / solve_sliced / solve_within
        solved, into the first n rows of the device tensor out [>= n, 8] (lam, grad: likewise, or None); launched behind whatever
        that call launched.  -> n; 0, and nothing launched, before the first of them.  What tells a fleet server whether a cut robot is
        worth a second slice: word 0 / word 3 of its record."""
        return self._inspect(self.eng.stationarity_device, out, lam=lam, grad=grad)

    def cost_terms(self, out, nodes=None):
        """The cost-breakdown records (DdpEngine.cost_terms_device) of the instances the last flush / solve_sliced / solve_within
        solved, into the first n rows of the device tensor out [>= n, 16] (nodes [>= n, N + 1, 14]: likewise, or None); launched behind
        whatever that call launched.  -> n; 0, and nothing launched, before the first of them.  What tells a fleet server which gain a
        fleet's cost is made of before it turns one."""
        return self._inspect(self.eng.cost_terms_device, out, nodes=nodes)

    def param_gradient(self, out, grad=None):
        """The parameter-sensitivity records (DdpEngine.param_gradient_device) of the instances the last flush / solve_sliced /
        solve_within solved, into the first n rows of the device tensor out [>= n, 8] (grad [>= n, N + 1, np]: likewise, or None);
        launched behind whatever that call launched.  -> n; 0, and nothing launched, before the first of them.  What tells a fleet
        server which way to move a reference or a foothold of each robot before the next tick."""
        return self._inspect(self.eng.param_gradient_device, out, grad=grad)

    def const_gradient(self, out, nodes=None):
        """The constant-sensitivity records (DdpEngine.const_gradient_device) of the instances the last flush / solve_sliced /
        solve_within solved, into the first n rows of the device tensor out [>= n, 40] (nodes [>= n, N + 1, 32]: likewise, or None);
        launched behind whatever that call launched.  -> n; 0, and nothing launched, before the first of them.  What tells a fleet
        server whose payload estimate its plans' costs are most sensitive to."""
        return self._inspect(self.eng.const_gradient_device, out, nodes=nodes)

    def policy_covariance(self, sigma0, out, q=None, r=None, cov=None, ucov_diag=None, start: int = 0, steps: int | None = None,
                          friction: float = 0.0):
        """The plan-uncertainty records (DdpEngine.policy_covariance_device) of the instances the last flush / solve_sliced /
        solve_within solved, from the first n rows of the device tensor sigma0 [>= n, nx, nx] (q [>= n, nx], r [>= n, nu]: likewise, or
        None) into the first n rows of out [>= n, 16] (cov [>= n, steps + 1, nx, nx], ucov_diag [>= n, steps, nu]: likewise, or None);
        launched behind whatever that call launched (a queue with policy=True: behind its policy launch; without one the records say
        ok = 0 and the propagation is the open-loop one).  -> n; 0, and nothing launched, before the first of them.  What tells a
        fleet server which robots' plans do not absorb the estimator's noise."""
        def launch(o, first, n, sigma0, **opt):
            return self.eng.policy_covariance_device(sigma0, o, first=first, count=n, start=start, steps=steps, friction=friction, **opt)
        return self._inspect(launch, out, sigma0=sigma0, q=q, r=r, cov=cov, ucov_diag=ucov_diag)

    def value_at(self, x_meas, out, node: int = 0):
        """The cost-to-go records (DdpEngine.value_at_device) of the instances the last flush / solve_sliced / solve_within solved, at the
        first n rows of the device tensor x_meas [>= n, nx] (the states measured at node `node` of each plan) into the first n rows of
        out [>= n, 8]; launched behind whatever that call launched.  It needs the engine's enable_value and a queue with policy=True,
        whose policy launch fills the value records (without one they are zeros with ok = 0).  -> n; 0, and nothing launched, before the
        first of them.  What tells a fleet server, in cost units, whose plan a tick's measurements have invalidated most: word 0 - word 3
        of a record is the predicted cost increase, and ranks the robots for the next re-solve."""
        def launch(o, first, n, x_meas):
            return self.eng.value_at_device(x_meas, o, node=node, first=first, count=n)
        return self._inspect(launch, out, x_meas=x_meas)

    def solve_sliced(self, first_slice: int, max_iters: int):
        """The pending batches in two slices (resumable solves, include/sddp.h): ONE launch runs every instance for at most
        `first_slice` iterations and the first-knot records (u_0 | x_1 | cost | iterations) are packed behind it -- those of the
        finished instances are final and can be handed out at once; if any instance is unfinished, max_iters is raised and a
        second launch finishes the stragglers alone (a finished instance costs it one queue pull).  Every instance ends with
        exactly the bytes of one uncut solve at `max_iters`.
        -> (finished [n] bool device tensor: which instances the first slice finished; records [n, words] of all of them after the
        last slice).  `first_records` keeps the records packed behind the first slice.
        The records are always the "first_knot" ones and there is no collective and no policy launch, whatever `gather` / `policy`
        the queue was made with: the caller owns the two record tensors.  The engine is left as it was found (DdpEngine.
        cut_and_continue); a caller that slices every tick calls `engine.enable_resume()` once and saves the carry's allocation."""
        return self._cut_and_continue(total=max_iters, first_slice=first_slice)

    def solve_within(self, budget_us: float, total: int, min_iters: int = 0):
        """The pending batches under a TIME budget (time-budgeted launches, include/sddp.h): solve_sliced with the first slice
        cut by the device clock instead of an iteration count.  ONE launch at max_iters = `total` ends `budget_us` microseconds
        of device time after it started (every instance it runs gets at least `min_iters` iterations) and the first-knot records
        are packed behind it -- those of the finished instances are final; if any instance is unfinished, a second launch with
        the budget OFF finishes the stragglers alone.  Every instance ends with exactly the bytes of one uncut solve at `total`.
        -> (finished [n] bool device tensor: which instances the budgeted launch finished; records [n, words] of all of them
        after the last launch).  `first_records` keeps the records packed behind the first launch, `overrun_us` how far that launch
        ran past its deadline.  Records, collective, policy and the state of the engine as in solve_sliced."""
        return self._cut_and_continue(total=total, budget_us=budget_us, min_iters=min_iters)

    def _cut_and_continue(self, **cut):
        """the pending batches by DdpEngine.cut_and_continue, the records packed behind each launch -> (finished, records)"""
        import torch
        n = self.pending * self.batch
        if n == 0:
            return None, None
        eng = self.eng
        shape = (self.batch * self.depth, eng.record_words("first_knot"))
        if getattr(self, "_sliced", None) is None or self._sliced[0].shape != shape:
            self._sliced = [torch.empty(shape, dtype=torch.float64, device=self.x.device) for _ in range(2)]
        finished = records = None

        def between():
            nonlocal finished, records
            self.first_records = records = eng.pack_records_device(self._sliced[0][:n], 0, n, "first_knot")
            finished = self.si[:n, _lib.STATS_I32_STATUS] != 1

        def overrun():                               # before the second launch rewrites the slot times
            self.overrun_us = eng.deadline_overrun_us()

        def behind():
            nonlocal records
            records = eng.pack_records_device(self._sliced[1][:n], 0, n, "first_knot")

        more = eng.cut_and_continue(lambda: eng.solve_range_device(self.P, 0, n), count=n, params=self.P, between=between,
                                    drained=overrun if "budget_us" in cut else None, behind=behind, **cut)
        self.launches += 2 if more > 0 else 1
        self.pending = 0
        self.solved = n
        return finished, records

    def _wait(self, k):
        if self._work[k] is not None:
            self._work[k].wait()
            self._work[k] = None

    def wait(self):
        """Every outstanding collective has completed (on torch's current stream for RCCL) when this returns."""
        self._wait(0)
        self._wait(1)

    @property
    def gathered(self):
        """Records of every rank's last flush, rank-major [world * n, words] (a view of the gather buffer: valid until the flush
        after next).  Waits for that collective."""
        if self._last is None:
            return None
        self._wait(self._last)
        return self._out[self._last][:self.world * self._n[self._last]]
