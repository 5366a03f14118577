"""Batched DDP engine object: the Python face of one ``sddp_handle`` (include/sddp.h).

Stands where ``pyddp.DdpSolver`` stands in the reference (python/ddp.py:93-94): constructed once, kept across MPC
ticks, ``solve(params) -> (x, u)``, ``is_converged()``, ``set_initial_state``, ``set_x_warmstart``,
``set_u_warmstart`` -- widened from one problem to a batch of B independent problems (knot-major C ABI layout).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class DdpEngine:
    def __init__(self, model: str, N: int, batch: int = 1, opts: dict | None = None, consts: dict | None = None,
                 model_id: int | None = None):
        """model_id: a user build of `model` (srbd_horizon_amd/userterms.py register) instead of the model's own builds."""
        self.lib = _lib.load()
        self.model = model
        self.model_id = _lib.MODEL_IDS[model] if model_id is None else int(model_id)
        self.N, self.B = int(N), int(batch)
        self.nx, self.nu, self.np_ = _lib.model_dims(model)
        self.opts = _lib.default_options(**(opts or {}))
        self.consts = _lib.default_consts(model, **(consts or {}))
        self._instance_rows = []      # (first, SddpModelConsts[count]) of every set_instance_consts, in call order
        h = C.c_void_p()
        _lib.check(self.lib.sddp_create(C.byref(h), self.model_id, self.N, self.B,
                                        C.byref(self.opts), C.byref(self.consts)))
        self.h = h
        npar = C.c_int()                     # a handle with user rows (consts extra_rows) has MAX_EXTRA more parameter columns
        self._chk(self.lib.sddp_handle_dims(h, None, None, C.byref(npar)))
        self.np_ = npar.value
        self._keep = []
        self.resume_enabled = False

    # ---- lifetime ------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.sddp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        _lib.check(rc, self.h)

    def _count(self, first, count):
        """how many instances [first, first + count) are; count = None: all from `first` on"""
        return int(self.B - first if count is None else count)

    @staticmethod
    def _c(a, shape):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
        return a

    def set_options(self, **over):
        for k, v in over.items():
            if not hasattr(self.opts, k):
                raise KeyError(f"unknown option {k!r}")
            setattr(self.opts, k, v)
        self._chk(self.lib.sddp_set_options(self.h, C.byref(self.opts)))

    # ---- host (numpy) path: [B][N+1][nx] etc. -------------------------------------------------------------------------
    def set_initial_state(self, x0):
        a = self._c(x0, (self.B, self.nx))
        self._chk(self.lib.sddp_set_initial_state(self.h, _lib.ptr(a)))

    def set_x_warmstart(self, x):
        a = self._c(x, (self.B, self.N + 1, self.nx))
        self._chk(self.lib.sddp_set_x_warmstart(self.h, _lib.ptr(a)))

    def set_u_warmstart(self, u):
        a = self._c(u, (self.B, self.N, self.nu))
        self._chk(self.lib.sddp_set_u_warmstart(self.h, _lib.ptr(a)))

    def load(self, x0=None, x=None, u=None):
        """Initial state / warm start of every instance from host arrays (the host counterpart of load_range_device): the setters
        of the arguments given, in this order."""
        if x0 is not None:
            self.set_initial_state(x0)
        if x is not None:
            self.set_x_warmstart(x)
        if u is not None:
            self.set_u_warmstart(u)

    def _results(self):                           # host arrays for what a solve returns: x [B, N+1, nx], u [B, N, nu], stats [B]
        return np.empty((self.B, self.N + 1, self.nx)), np.empty((self.B, self.N, self.nu)), np.zeros(self.B, dtype=_lib.STATS_DTYPE)

    def solve(self, params):
        p = self._c(params, (self.B, self.N + 1, self.np_))
        x, u, st = self._results()
        self._chk(self.lib.sddp_solve(self.h, _lib.ptr(p), _lib.ptr(x), _lib.ptr(u), _lib.ptr(st)))
        self.stats = st
        return x, u

    # ---- receding horizon with device-resident parameters / warm start -----------------------------
    def set_params(self, params):
        p = self._c(params, (self.B, self.N + 1, self.np_))
        self._chk(self.lib.sddp_set_params(self.h, _lib.ptr(p)))

    def advance(self, p_last, x0):
        """One tick on the device: parameters and previous solution shifted back by one knot, ``p_last`` written at node N,
        ``x0`` set as the initial state."""
        pl = self._c(p_last, (self.B, self.np_))
        x = self._c(x0, (self.B, self.nx))
        self._chk(self.lib.sddp_advance(self.h, _lib.ptr(pl), _lib.ptr(x)))

    def model_step(self, x, u, p, k: int = 0):
        """x_next = f_k(x, u; p) per instance through the solver's device model code (simulator step, dsrbd_example.py:158-159)."""
        xv = self._c(x, (self.B, self.nx)); uv = self._c(u, (self.B, self.nu)); pv = self._c(p, (self.B, self.np_))
        out = np.empty((self.B, self.nx))
        self._chk(self.lib.sddp_model_step(self.h, _lib.ptr(xv), _lib.ptr(uv), _lib.ptr(pv), int(k), _lib.ptr(out)))
        return out

    def solve_resident(self):
        x, u, st = self._results()
        self._chk(self.lib.sddp_solve_resident(self.h, _lib.ptr(x), _lib.ptr(u), _lib.ptr(st)))
        self.stats = st
        return x, u

    def solve_resident_first(self, policy: bool = False):
        """One tick of a fleet in closed loop: solve on the resident data, fetch only u_0 [B,nu], x_1 [B,nx], cost, iterations and
        status per robot (the trajectories stay on the device as the next warm start).  -> (u0, x1); self.first_stats
        policy=True (needs enable_policy): one policy launch behind the solve; -> (u0, x1, K0 [B,nu,nx]), the feedback gains of the
        first knot at the returned iterate; self.first_policy = (kff, K, info) of every kept knot."""
        u0 = np.empty((self.B, self.nu))
        x1 = np.empty((self.B, self.nx))
        cost = np.empty(self.B)
        iters = np.empty(self.B, dtype=np.int32)
        status = np.empty(self.B, dtype=np.int32)
        self._chk(self.lib.sddp_solve_resident_first(self.h, _lib.ptr(u0), _lib.ptr(x1), _lib.ptr(cost), _lib.ptr(iters), _lib.ptr(status)))
        self.first_stats = dict(cost=cost, iters=iters, status=status)
        if policy:
            self.policy_range_device()
            self.first_policy = self.policy()
            return u0, x1, self.first_policy[1][:, 0].copy()
        return u0, x1

    # ---- policy export: the feedback policy u_k + K_k (x - x_k) of the RETURNED iterate (include/sddp.h) -------------------------
    def enable_policy(self, knots: int):
        """Allocate the per-instance policy buffer for the first `knots` knots (1..N; 0 frees it)."""
        self._chk(self.lib.sddp_enable_policy(self.h, int(knots)))

    def policy_words(self):
        """-> (doubles per instance record, knots kept)"""
        w, k = C.c_int(), C.c_int()
        self._chk(self.lib.sddp_policy_words(self.h, C.byref(w), C.byref(k)))
        return w.value, k.value

    def policy_range_device(self, first: int = 0, count: int | None = None):
        """One sweep per instance of [first, first + count) at the iterate the last solve returned; asynchronous, behind the solve."""
        self._chk(self.lib.sddp_policy_range_device(self.h, int(first), self._count(first, count)))

    def fetch_policy(self, first: int = 0, count: int | None = None):
        """The raw policy records [count, words] of the last policy launch (waits for the stream)."""
        n = self._count(first, count)
        out = np.empty((max(n, 0), self.policy_words()[0]))
        self._chk(self.lib.sddp_fetch_policy(self.h, int(first), n, _lib.ptr(out)))
        return out

    def split_policy(self, rec):
        """records [n, words] -> (kff [n, M, nu], K [n, M, nu, nx], info [n, 4] = mu_used, theta_used, expected, ok)"""
        n, M = rec.shape[0], (rec.shape[1] - 4) // (self.nu * (self.nx + 1))
        g = rec[:, :-4].reshape(n, M, self.nu * (self.nx + 1))
        return g[:, :, :self.nu].copy(), g[:, :, self.nu:].reshape(n, M, self.nu, self.nx).copy(), rec[:, -4:].copy()

    def policy(self, first: int = 0, count: int | None = None):
        """-> (kff [n, M, nu], K [n, M, nu, nx], info [n, 4]) of the instances [first, first + count), as the last policy launch
        (policy_range_device) left them: the gains of the sweep at the RETURNED iterate, u = u_k + kff_k + K_k (x - x_k) being the
        solver's next step and u_k + K_k (x - x_k) the feedback law around the plan."""
        return self.split_policy(self.fetch_policy(first, count))

    def apply_policy_device(self, x_meas, u_out, first: int = 0, count: int | None = None, knot: int = 0):
        """u_out[i] = u_k[b] + K_k[b] (x_meas[i] - x_k[b]), b = first + i, k = knot < the knots kept: device tensors [count, nx] ->
        [count, nu]; asynchronous."""
        n = self._count(first, count)
        xm, uo = self._dev(x_meas, (n, self.nx)), self._dev(u_out, (n, self.nu))
        if knot == 0:
            self._chk(self.lib.sddp_apply_policy_device(self.h, int(first), n, xm, uo))
        else:
            self._chk(self.lib.sddp_apply_policy_knot_device(self.h, int(first), n, int(knot), xm, uo))
        return u_out

    def policy_rollout_device(self, x_meas, x_out, u_out, cost_out=None, first: int = 0, count: int | None = None, start: int = 0,
                              steps: int | None = None):
        """The exported policy rolled out through the solver's device model from the measured states x_meas [count, nx] at node
        `start`: x_out [count, steps + 1, nx] (row 0 = x_meas), u_out [count, steps, nu] with u_j = u_k + K_k (x_j - x_k), k = start + j,
        cost_out [count] or None: the stage costs along it, summed.  Device tensors; steps None: to the last kept knot.  Asynchronous,
        behind the solve and the policy launch."""
        n = self._count(first, count)
        s = int(self.policy_words()[1] - start if steps is None else steps)
        rows = max(s, 0)                      # (a refused steps < 1 reaches the library, which says what is allowed)
        self._chk(self.lib.sddp_policy_rollout_device(self.h, int(first), n, int(start), s, self._dev(x_meas, (n, self.nx)),
                                                      self._dev(x_out, (n, rows + 1, self.nx)), self._dev(u_out, (n, rows, self.nu)),
                                                      self._dev_or_null(cost_out, (n,))))
        return x_out, u_out, cost_out

    def policy_rollout(self, x_meas, first: int = 0, count: int | None = None, start: int = 0, steps: int | None = None):
        """policy_rollout_device from and to numpy: x_meas [n, nx] -> (x [n, steps + 1, nx], u [n, steps, nu], cost [n]); waits for
        the stream."""
        import torch
        n = self._count(first, count)
        s = int(self.policy_words()[1] - start if steps is None else steps)
        xm = torch.from_numpy(self._c(x_meas, (n, self.nx))).cuda()
        return self._to_numpy(n, [(max(s, 0) + 1, self.nx), (max(s, 0), self.nu), ()],
                              lambda x, u, cost: self.policy_rollout_device(xm, x, u, cost, first, n, start, s))

    def policy_covariance_device(self, sigma0, out, q=None, r=None, cov=None, ucov_diag=None, first: int = 0, count: int | None = None,
                                 start: int = 0, steps: int | None = None, friction: float = 0.0):
        """The covariance of the state under the exported policy, linearised along the plan (include/sddp.h, "plan uncertainty"):
        from sigma0 [count, nx, nx] at node `start` (symmetric; its lower triangle is read), S_{j+1} = A_k S_j A_k^T + B_k diag(r) B_k^T +
        diag(q) with A_k = f_x + f_u K_k, B_k = f_u, k = start + j.  out [count, POLICY_COV_WORDS]: the records (_lib.POLICY_COV_* words;
        word 0 the smallest cone margin of a stance force in standard deviations).  q [count, nx] / r [count, nu]: process / actuation
        variances, or None: 0.  cov [count, steps + 1, nx, nx] (row j = S_j) / ucov_diag [count, steps, nu] (row j = diag K_k S_j K_k^T),
        or None.  Device tensors; steps None: to the last kept knot.  friction > 0: the ground's coefficient for this call, else the
        handle's.  Asynchronous, behind the solve and the policy launch."""
        n = self._count(first, count)
        s = int(self.policy_words()[1] - start if steps is None else steps)
        rows = max(s, 0)                      # (a refused steps < 1 reaches the library, which says what is allowed)
        self._chk(self.lib.sddp_policy_covariance_device(
            self.h, int(first), n, int(start), s, self._dev(sigma0, (n, self.nx, self.nx)), self._dev_or_null(q, (n, self.nx)),
            self._dev_or_null(r, (n, self.nu)), float(friction), self._dev(out, (n, _lib.POLICY_COV_WORDS)),
            self._dev_or_null(cov, (n, rows + 1, self.nx, self.nx)), self._dev_or_null(ucov_diag, (n, rows, self.nu))))
        return out

    def policy_covariance(self, sigma0, q=None, r=None, first: int = 0, count: int | None = None, start: int = 0, steps: int | None = None,
                          friction: float = 0.0):
        """policy_covariance_device from and to numpy: sigma0 [n, nx, nx], q [n, nx] or None, r [n, nu] or None ->
        dict(record [n, POLICY_COV_WORDS], cov [n, steps + 1, nx, nx], ucov_diag [n, steps, nu]); waits for the stream."""
        import torch
        n = self._count(first, count)
        s = int(self.policy_words()[1] - start if steps is None else steps)
        up = lambda a, shape: None if a is None else torch.from_numpy(self._c(a, shape)).cuda()      # noqa: E731
        s0, dq, dr = up(sigma0, (n, self.nx, self.nx)), up(q, (n, self.nx)), up(r, (n, self.nu))
        rec, cov, ud = self._to_numpy(n, [(_lib.POLICY_COV_WORDS,), (max(s, 0) + 1, self.nx, self.nx), (max(s, 0), self.nu)],
                                      lambda out, cv, uc: self.policy_covariance_device(s0, out, dq, dr, cv, uc, first, n, start, s, friction))
        return dict(record=rec, cov=cov, ucov_diag=ud)

    # ---- cost-to-go export: the value function per node out of the policy sweep (include/sddp.h, "cost-to-go export") ------------
    def enable_value(self, nodes: int):
        """Allocate the per-instance value buffer for the nodes 0 .. nodes - 1 (1..N+1; 0 frees it).  Needs enable_policy first: every
        policy_range_device then stores the value records of its range in the same launch."""
        self._chk(self.lib.sddp_enable_value(self.h, int(nodes)))

    def value_words(self):
        """-> (doubles per instance record, nodes kept)"""
        w, k = C.c_int(), C.c_int()
        self._chk(self.lib.sddp_value_words(self.h, C.byref(w), C.byref(k)))
        return w.value, k.value

    def fetch_value(self, first: int = 0, count: int | None = None):
        """The raw value records [count, nodes, nx * nx + nx + 2] of the last policy launch, on the host (waits for the stream)."""
        n = self._count(first, count)
        nodes = self.value_words()[1]
        out = np.empty((max(n, 0), nodes, _lib.value_node_words(self.nx)))
        self._chk(self.lib.sddp_fetch_value(self.h, int(first), n, _lib.ptr(out)))
        return out

    def value(self, first: int = 0, count: int | None = None):
        """-> dict of CUDA tensors c [n, nodes], expected [n, nodes], vx [n, nodes, nx], Vxx [n, nodes, nx, nx] of the instances
        [first, first + count), as the last policy launch left them: V_k(x_k + d) ~ c_k + expected_k + vx_k . d + 1/2 d^T Vxx_k d, the
        sweep's own (Gauss-Newton) model.  Copies of the handle's buffer; waits for the stream."""
        n = self._count(first, count)
        nodes = self.value_words()[1]
        if n < 1 or first < 0 or first > self.B - n:
            raise ValueError("instance range outside the batch")
        self.synchronize()
        rec = self.device_view(_lib.DEVICE_BUF_VALUE, (self.B, nodes, _lib.value_node_words(self.nx)))[first:first + n]
        nx = self.nx
        return dict(c=rec[:, :, 0].clone(), expected=rec[:, :, 1].clone(), vx=rec[:, :, 2:2 + nx].clone(),
                    Vxx=rec[:, :, 2 + nx:].reshape(n, nodes, nx, nx).clone())

    def value_at_device(self, x_meas, out, node: int = 0, first: int = 0, count: int | None = None):
        """The value record of node `node` evaluated at the measured states x_meas [count, nx] -> out [count, VALUE_AT_WORDS]
        (_lib.VALUE_AT_FIELDS: value, lin, quad, c, expected, |delta|_inf, ok, node).  Device tensors; asynchronous, behind the solve and
        the policy launch."""
        n = self._count(first, count)
        self._chk(self.lib.sddp_value_at_device(self.h, int(first), n, int(node), self._dev(x_meas, (n, self.nx)),
                                                self._dev(out, (n, _lib.VALUE_AT_WORDS))))
        return out

    def value_at(self, x_meas, node: int = 0, first: int = 0, count: int | None = None):
        """value_at_device for x_meas [n, nx] as a CUDA tensor (-> a CUDA tensor [n, VALUE_AT_WORDS], asynchronous) or as a numpy array
        (-> numpy; waits for the stream)."""
        import torch
        n = self._count(first, count)
        if isinstance(x_meas, torch.Tensor):
            return self.value_at_device(x_meas, torch.empty((max(n, 0), _lib.VALUE_AT_WORDS), dtype=torch.float64, device="cuda"), node, first, n)
        xm = torch.from_numpy(self._c(x_meas, (n, self.nx))).cuda()
        return self._to_numpy(n, [(_lib.VALUE_AT_WORDS,)], lambda out: self.value_at_device(xm, out, node, first, n))[0]

    # ---- the plan inspectors: audit, stationarity certificate, cost breakdown, parameter and constant sensitivities ("Plan inspectors") ----------------
    # Each reads the instances [first, first + count) of a handle that has solved: the handle's own plan (x, u None) or the caller's
    # device tensors, whose block i belongs to instance first + i.  Every build has them; the *_device forms are asynchronous,
    # behind the solve, and store to nothing but their outputs.
    def _plan(self, n, x, u, steps=None):
        """the trajectory pointers of an inspector: x [n, steps + 1, nx], u [n, steps, nu] (steps None: N), or None: NULL"""
        if x is None and u is None:
            return None, None                  # the handle's own plan
        steps = self.N if steps is None else max(steps, 0)      # (a refused steps < 1 reaches the library, which says what is allowed)
        return self._dev_or_null(x, (n, steps + 1, self.nx)), self._dev_or_null(u, (n, steps, self.nu))

    def _to_numpy(self, n, shapes, run):
        """run(*t) on fresh float64 CUDA tensors t[j] of shape [max(n, 0), *shapes[j]]; waits for the stream -> them as numpy arrays"""
        import torch
        ts = [torch.empty((max(n, 0), *shape), dtype=torch.float64, device="cuda") for shape in shapes]
        run(*ts)
        self.synchronize()
        return tuple(t.cpu().numpy() for t in ts)

    def _own_records(self, fn, first, count, words, *args):
        """the host-array twin `fn` of an inspector: the records [count, words] of the handle's own plan; waits for the stream"""
        n = self._count(first, count)
        out = np.empty((max(n, 0), words))
        self._chk(fn(self.h, int(first), n, *args, _lib.ptr(out)))
        return out

    def audit_device(self, out, first: int = 0, count: int | None = None, x=None, u=None, start: int = 0, steps: int | None = None,
                     friction: float = 0.0):
        """The audit records (_lib.AUDIT_* words) of the instances [first, first + count) into the device tensor out
        [count, AUDIT_WORDS].  x, u None: the handle's own plan; else device tensors x [count, steps + 1, nx], u [count, steps, nu]
        whose row j sits at node start + j (the outputs of policy_rollout_device); steps None: to node N.  friction > 0: the ground's
        coefficient for this call, else the handle's friction_cone_coefficient."""
        n = self._count(first, count)
        s = int(self.N - start if steps is None else steps)
        self._chk(self.lib.sddp_audit_range_device(self.h, int(first), n, int(start), s, *self._plan(n, x, u, s), float(friction),
                                                   self._dev(out, (n, _lib.AUDIT_WORDS))))
        return out

    def audit(self, first: int = 0, count: int | None = None, friction: float = 0.0):
        """The audit records [count, AUDIT_WORDS] of the handle's own plan as a numpy array; waits for the stream."""
        return self._own_records(self.lib.sddp_audit, first, count, _lib.AUDIT_WORDS, float(friction))

    def stationarity_device(self, out, first: int = 0, count: int | None = None, x=None, u=None, lam=None, grad=None):
        """The stationarity records (_lib.STATIONARITY_FIELDS) of the instances [first, first + count) into the device tensor out
        [count, 8].  x, u None: the handle's own plan; else device tensors x [count, N + 1, nx], u [count, N, nu], a caller's
        whole-horizon trajectory.  lam [count, N + 1, nx] / grad [count, N, nu]: device tensors for every costate / reduced gradient,
        or None."""
        n = self._count(first, count)
        self._chk(self.lib.sddp_stationarity_range_device(self.h, int(first), n, *self._plan(n, x, u),
                                                          self._dev(out, (n, len(_lib.STATIONARITY_FIELDS))), *self._plan(n, lam, grad)))
        return out

    def stationarity(self, first: int = 0, count: int | None = None, full: bool = False):
        """The stationarity records [count, 8] of the handle's own plan as a numpy array; full: -> (records, lambda [count, N + 1, nx],
        s [count, N, nu]).  Waits for the stream."""
        words = len(_lib.STATIONARITY_FIELDS)
        if not full:
            return self._own_records(self.lib.sddp_stationarity, first, count, words)
        n = self._count(first, count)
        return self._to_numpy(n, [(words,), (self.N + 1, self.nx), (self.N, self.nu)],
                              lambda out, lam, grad: self.stationarity_device(out, first, n, lam=lam, grad=grad))

    def cost_terms_device(self, out, first: int = 0, count: int | None = None, x=None, u=None, nodes=None):
        """The cost-breakdown records of the instances [first, first + count) into the device tensor out [count, 16]: total | the 13
        families of _lib.COST_TERM_NAMES | the largest of the families 0 .. 11 | N.  x, u None: the handle's own plan; else device
        tensors x [count, N + 1, nx], u [count, N, nu], a caller's whole-horizon trajectory.  nodes [count, N + 1, 14]: a device tensor
        for the per-node addends (column 0 the total, column 1 + f family f), or None."""
        n = self._count(first, count)
        self._chk(self.lib.sddp_cost_terms_range_device(self.h, int(first), n, *self._plan(n, x, u), self._dev(out, (n, _lib.COST_TERMS_WORDS)),
                                                        self._dev_or_null(nodes, (n, self.N + 1, _lib.COST_TERMS_COLS))))
        return out

    def cost_terms(self, first: int = 0, count: int | None = None, nodes: bool = False):
        """The cost breakdown of the handle's own plan as a dict of numpy arrays: "total" [count], one entry [count] per family name
        of _lib.COST_TERM_NAMES, "largest" [count] (the name of the largest of the families 0 .. 11, "" where one of them is NaN) and
        "record" [count, 16], the raw records; nodes: also "nodes" [count, N + 1, 14], the per-node addends.  Waits for the stream."""
        names, per_node = _lib.COST_TERM_NAMES, {}
        if not nodes:
            rec = self._own_records(self.lib.sddp_cost_terms, first, count, _lib.COST_TERMS_WORDS)
        else:
            n = self._count(first, count)
            rec, per_node["nodes"] = self._to_numpy(n, [(_lib.COST_TERMS_WORDS,), (self.N + 1, _lib.COST_TERMS_COLS)],
                                                    lambda out, nd: self.cost_terms_device(out, first, n, nodes=nd))
        return {"total": rec[:, 0].copy(), **{name: rec[:, 1 + f].copy() for f, name in enumerate(names)},
                "largest": np.array([names[int(i)] if i >= 0 else "" for i in rec[:, 14]], dtype=object), "record": rec, **per_node}

    def param_gradient_device(self, out, first: int = 0, count: int | None = None, x=None, u=None, grad=None, lam=None):
        """The parameter-sensitivity records (_lib.PARAM_GRADIENT_FIELDS) of the instances [first, first + count) into the device
        tensor out [count, 8].  x, u None: the handle's own plan; else device tensors x [count, N + 1, nx], u [count, N, nu], a caller's
        whole-horizon trajectory.  grad [count, N + 1, np]: a device tensor for every G_k = dL_k/dp_k + (df_k/dp_k)^T lambda_{k+1}, np
        the handle's parameter width; lam [count, N + 1, nx]: one for the costates, the bits of stationarity_device's; or None."""
        n = self._count(first, count)
        self._chk(self.lib.sddp_param_gradient_range_device(self.h, int(first), n, *self._plan(n, x, u),
                                                            self._dev(out, (n, len(_lib.PARAM_GRADIENT_FIELDS))),
                                                            self._dev_or_null(grad, (n, self.N + 1, self.np_)),
                                                            self._dev_or_null(lam, (n, self.N + 1, self.nx))))
        return out

    def param_gradient(self, first: int = 0, count: int | None = None, x=None, u=None, want_lambda: bool = False):
        """The gradient of each plan's cost in its per-knot parameters, on the device: x, u None (the handle's own plan) or device
        tensors as for param_gradient_device -> (grad [count, N + 1, np], record [count, 8]), with want_lambda also lambda
        [count, N + 1, nx] whose row 0 is the gradient in x_0; fresh float64 CUDA tensors.  Asynchronous, behind the solve: synchronize()
        (or a copy to the host) before reading.  At a converged plan with closed gaps grad is the gradient of the optimal cost in P;
        record words "stationarity" and "defect" say how far from that the plan is."""
        import torch
        n = self._count(first, count)
        mk = lambda *shape: torch.empty((max(n, 0), *shape), dtype=torch.float64, device="cuda")      # noqa: E731
        rec, grad = mk(len(_lib.PARAM_GRADIENT_FIELDS)), mk(self.N + 1, self.np_)
        lam = mk(self.N + 1, self.nx) if want_lambda else None
        self.param_gradient_device(rec, first, n, x=x, u=u, grad=grad, lam=lam)
        return (grad, rec, lam) if want_lambda else (grad, rec)

    def const_gradient_device(self, out, first: int = 0, count: int | None = None, x=None, u=None, nodes=None, lam=None):
        """The constant-sensitivity records of the instances [first, first + count) into the device tensor out [count, 40]: the 32
        columns of _lib.CONST_GRADIENT_NAMES (the gradient of the plan's cost in the derived constants the kernels read), then the
        words _lib.CONST_GRADIENT_TAIL.  x, u None: the handle's own plan; else device tensors x [count, N + 1, nx], u [count, N, nu], a
        caller's whole-horizon trajectory.  nodes [count, N + 1, 32]: a device tensor for the per-node addends, whose in-order column
        sums the record's columns are; lam [count, N + 1, nx]: one for the costates, the bits of stationarity_device's; or None."""
        n = self._count(first, count)
        self._chk(self.lib.sddp_const_gradient_range_device(self.h, int(first), n, *self._plan(n, x, u),
                                                            self._dev(out, (n, _lib.CONST_GRADIENT_WORDS)),
                                                            self._dev_or_null(nodes, (n, self.N + 1, _lib.CONST_GRADIENT_COLS)),
                                                            self._dev_or_null(lam, (n, self.N + 1, self.nx))))
        return out

    def instance_consts(self, b: int):
        """the constants instance b is solved with: its row of set_instance_consts, else the handle's own"""
        for first, rows in reversed(self._instance_rows):      # the last call that covers b holds its row
            if first <= int(b) < first + len(rows):
                return rows[int(b) - first]
        return self.consts

    def const_gradient_fields(self, derived, b: int = 0):
        """words 0 .. 31 of a constant-sensitivity record of instance b -> a dict by sddp_model_consts field name (m, I [9], com [3],
        feet [12], dt, force_scaling, the gains, lip_height, the barrier constants): the chain rule of sddp_const_gradient_fields with
        the constants the engine holds for that instance.  Host code alone."""
        c = self.instance_consts(b)
        d = np.ascontiguousarray(derived, dtype=np.float64).reshape(-1)[:_lib.CONST_GRADIENT_COLS].copy()
        out, n = np.zeros(len(_lib.CONST_GRADIENT_FIELD_NAMES)), C.c_int()
        if self.lib.sddp_const_gradient_fields(C.byref(c), _lib.ptr(d), _lib.ptr(out), C.byref(n)) != 0:
            raise RuntimeError((self.lib.sddp_last_error(None) or b"").decode())
        fields = {}
        for name, v in zip(_lib.CONST_GRADIENT_FIELD_NAMES, out):
            base = name.split("[")[0]
            if base == name:
                fields[name] = float(v)
            else:
                fields.setdefault(base, []).append(float(v))
        return {k: (np.array(v) if isinstance(v, list) else v) for k, v in fields.items()}

    def const_gradient(self, first: int = 0, count: int | None = None, x=None, u=None, nodes: bool = False):
        """The gradient of each plan's cost in the robot's constants, on the device: x, u None (the handle's own plan) or device tensors
        as for const_gradient_device -> (record [count, 40] as a numpy array, [count] dicts by sddp_model_consts field name, each through
        const_gradient_fields with that instance's own constants); nodes: also the addends [count, N + 1, 32].  Waits for the stream.
        At a converged plan with closed gaps it is the gradient of the optimal cost; the record's words "stationarity" and "defect" say
        how far from that the plan is."""
        n = self._count(first, count)
        shapes = [(_lib.CONST_GRADIENT_WORDS,)] + ([(self.N + 1, _lib.CONST_GRADIENT_COLS)] if nodes else [])
        got = self._to_numpy(n, shapes, lambda out, nd=None: self.const_gradient_device(out, first, n, x=x, u=u, nodes=nd))
        fields = [self.const_gradient_fields(got[0][i], first + i) for i in range(got[0].shape[0])]
        return (got[0], fields, got[1]) if nodes else (got[0], fields)

    def is_converged(self):
        f = np.zeros(self.B, dtype=np.int32)
        self._chk(self.lib.sddp_is_converged(self.h, _lib.ptr(f)))
        return f.astype(bool)

    # ---- phase-level entry points (parity tests) ---------------------------------------------------------------------------
    def _phase_mode(self, theta=0.0, closed=False):
        self._chk(self.lib.sddp_debug_set_phase_mode(self.h, float(theta), int(bool(closed))))

    def backward(self, params, mu=0.0, theta=0.0, closed=False):
        """One sweep at the handle's trajectory.  theta: weight of the second-order term (a solve's sweep after a full step runs
        theta = 1); closed: the closed-gap path, all defects taken as zero (one-wave kernels only).  The mode holds for this call."""
        p = self._c(params, (self.B, self.N + 1, self.np_))
        gains = np.empty((self.B, self.N, self.nu * (self.nx + 1)))
        scal = np.empty((self.B, 8))
        self._phase_mode(theta, closed)
        try:
            self._chk(self.lib.sddp_backward(self.h, _lib.ptr(p), float(mu), _lib.ptr(gains), _lib.ptr(scal)))
        finally:
            self._phase_mode()
        kff = gains[:, :, :self.nu]
        K = gains[:, :, self.nu:].reshape(self.B, self.N, self.nu, self.nx)
        return kff, K, scal

    def forward(self, params, alpha, closed=False):
        """One rollout with the gains of the last backward(); closed: without the (1 - alpha) d correction (one-wave kernels only)."""
        p = self._c(params, (self.B, self.N + 1, self.np_))
        x = np.empty((self.B, self.N + 1, self.nx))
        u = np.empty((self.B, self.N, self.nu))
        cost = np.empty(self.B)
        self._phase_mode(0.0, closed)
        try:
            self._chk(self.lib.sddp_forward(self.h, _lib.ptr(p), float(alpha), _lib.ptr(x), _lib.ptr(u), _lib.ptr(cost)))
        finally:
            self._phase_mode()
        return x, u, cost

    # ---- HBM-resident path (torch tensors on the GPU; PyTorch is plumbing for device memory and streams) ------------------
    def _dev(self, t, shape):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
            raise ValueError("expected a contiguous float64 CUDA tensor")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return C.c_void_p(t.data_ptr())

    def use_torch_stream(self, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        self._chk(self.lib.sddp_set_stream(self.h, C.c_void_p(s.cuda_stream)))

    def set_initial_state_device(self, x0):
        self._chk(self.lib.sddp_set_initial_state_device(self.h, self._dev(x0, (self.B, self.nx))))

    def set_x_warmstart_device(self, x):
        self._chk(self.lib.sddp_set_x_warmstart_device(self.h, self._dev(x, (self.B, self.N + 1, self.nx))))

    def set_u_warmstart_device(self, u):
        self._chk(self.lib.sddp_set_u_warmstart_device(self.h, self._dev(u, (self.B, self.N, self.nu))))

    def solve_device(self, params):
        """Asynchronous launch on the handle's stream; results stay in the handle's HBM buffers."""
        self._chk(self.lib.sddp_solve_device(self.h, self._dev(params, (self.B, self.N + 1, self.np_))))

    def synchronize(self):
        self._chk(self.lib.sddp_synchronize(self.h))

    def enable_timing(self, on=True):
        self._chk(self.lib.sddp_enable_timing(self.h, int(on)))

    def last_kernel_ms(self):
        ms = C.c_double()
        self._chk(self.lib.sddp_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def kernel_time_stats(self, reset=False):
        """(sum_ms, count) of the solve-kernel durations measured with HIP events on the handle's stream."""
        sm, n = C.c_double(), C.c_longlong()
        self._chk(self.lib.sddp_kernel_time_stats(self.h, C.byref(sm), C.byref(n), int(reset)))
        return sm.value, n.value

    def device_buffer(self, which: int):
        """(device pointer, bytes) of the buffer with the id `which`: one of _lib.BUF_* (include/sddp.h SDDP_BUF_*)"""
        p, n = C.c_void_p(), C.c_longlong()
        self._chk(self.lib.sddp_device_ptr(self.h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def device_view(self, which: int, shape=None, typestr="<f8"):
        """Zero-copy torch view of device_buffer(which); shape None: the whole buffer, flat.  No synchronisation: ordered behind the
        handle's stream like any torch work on it."""
        import torch
        ptr, nbytes = self.device_buffer(which)
        shape = (nbytes // int(typestr[2:]),) if shape is None else tuple(shape)

        class _Dev:
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2}

        return torch.as_tensor(_Dev(), device=torch.device("cuda", torch.cuda.current_device()))

    def _host_copy(self, which, typestr):
        """device_buffer(which), whole, as a host array; waits for the stream"""
        self.synchronize()
        return self.device_view(which, None, typestr).cpu().numpy().copy()

    def fetch_device_views(self):
        """Zero-copy torch views of the handle's HBM buffers: x [B,N+1,nx], u [B,N,nu], stats as f64 [B,8] and i32 [B,16]
        (sddp_stats: cost, alpha, gap, mu, expected, rho | iters, converged, status, rollouts = the last four i32 words;
        _lib.STATS_I32_ITERS etc.)."""
        return (self.device_view(_lib.BUF_XS, (self.B, self.N + 1, self.nx)), self.device_view(_lib.BUF_US, (self.B, self.N, self.nu)),
                self.device_view(_lib.BUF_STATS, (self.B, _lib.STATS_F64_WORDS)),
                self.device_view(_lib.BUF_STATS, (self.B, _lib.STATS_I32_WORDS), "<i4"))

    def fetch(self):
        """Copy the solution and stats of the last device solve to host numpy arrays (waits for the handle's stream)."""
        x, u, st = self._results()
        self._chk(self.lib.sddp_fetch(self.h, _lib.ptr(x), _lib.ptr(u), _lib.ptr(st)))
        self.stats = st
        return x, u, st

    # ---- the handle as a queue of instances (more instances than resident workgroups: one launch, work queue) -----------------
    def _dev_or_null(self, t, shape):
        return C.c_void_p(None) if t is None else self._dev(t, shape)

    def load_range_device(self, first: int, count: int, x0=None, x=None, u=None):
        """Initial state / warm start of the instances [first, first + count) from device tensors of `count` instances."""
        self._chk(self.lib.sddp_load_range_device(self.h, int(first), int(count), self._dev_or_null(x0, (count, self.nx)),
                                                  self._dev_or_null(x, (count, self.N + 1, self.nx)),
                                                  self._dev_or_null(u, (count, self.N, self.nu))))

    def solve_range_device(self, params, first: int, count: int):
        """One asynchronous launch over the instances [first, first + count); `params` is the whole [B, N+1, np] tensor."""
        self._chk(self.lib.sddp_solve_range_device(self.h, self._dev(params, (self.B, self.N + 1, self.np_)), int(first), int(count)))

    # ---- masked launches: solve, continue, export and advance any subset of a range (include/sddp.h) ---------------------------
    @staticmethod
    def _mask(mask, count):
        """the device pointer of a mask: a contiguous int32 CUDA tensor of `count` words, non-zero = selected"""
        import torch
        if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.int32 and mask.is_contiguous()):
            raise ValueError("expected a contiguous int32 CUDA tensor as the mask")
        if tuple(mask.shape) != (count,):
            raise ValueError(f"expected a mask of shape {(count,)}, got {tuple(mask.shape)}")
        return C.c_void_p(mask.data_ptr())

    def _params_or_resident(self, params):
        if params is None:
            return C.c_void_p(self.device_buffer(_lib.BUF_PARAMS)[0])
        return self._dev(params, (self.B, self.N + 1, self.np_))

    def solve_masked_device(self, params, mask, first: int = 0, count: int | None = None):
        """One asynchronous launch over the instances of [first, first + count) that `mask` selects (int32 device tensor [count],
        non-zero = selected): each gets what solve_range_device gives it, bit for bit; every other instance is untouched.  params:
        the whole [B, N+1, np] device tensor, None = the resident one.  No host synchronisation."""
        n = self._count(first, count)
        self._chk(self.lib.sddp_solve_masked_device(self.h, self._params_or_resident(params), int(first), n, self._mask(mask, n)))

    def continue_masked(self, mask, params=None, first: int = 0, count: int | None = None):
        """continue_solve for the selected instances alone: those that are selected and unfinished are taken up where they stopped."""
        n = self._count(first, count)
        self._chk(self.lib.sddp_continue_masked_device(self.h, self._params_or_resident(params), int(first), n, self._mask(mask, n)))

    def policy_masked_device(self, mask, first: int = 0, count: int | None = None):
        """policy_range_device for the selected instances alone; the records (and value records) of the others keep their bytes."""
        n = self._count(first, count)
        self._chk(self.lib.sddp_policy_masked_device(self.h, int(first), n, self._mask(mask, n)))

    def advance_masked_device(self, mask, p_last, x0, first: int = 0, count: int | None = None):
        """advance() for the selected instances alone, from device tensors p_last [count, np] and x0 [count, nx] indexed like the
        mask (rows of unselected instances are not read); their resume flags are cleared.  Asynchronous."""
        n = self._count(first, count)
        self._chk(self.lib.sddp_advance_masked_device(self.h, int(first), n, self._mask(mask, n), self._dev(p_last, (n, self.np_)),
                                                      self._dev(x0, (n, self.nx))))

    def last_selected(self) -> int:
        """How many instances the last masked solve / continue launch selected (waits for the stream)."""
        n = C.c_int()
        self._chk(self.lib.sddp_last_selected(self.h, C.byref(n)))
        return n.value

    # ---- resumable solves: continue a solve cut at max_iters, bit for bit (include/sddp.h) -------------------------------------
    def enable_resume(self, on: bool = True):
        """Every later solve launch of the handle can be continued: an instance that ends with status 1 (max_iters) keeps what the
        iteration carries.  Plain builds only (no barrier, no second_order = 2, no user rows)."""
        self._chk(self.lib.sddp_enable_resume(self.h, int(bool(on))))
        self.resume_enabled = bool(on)

    def continue_solve(self, params=None, first: int = 0, count: int | None = None):
        """One asynchronous launch that takes up the unfinished instances (status 1) of [first, first + count) where they stopped and
        runs them while iters < max_iters -- the TOTAL cap: raise it with set_options(max_iters=...) first.  Every other instance
        is left untouched.  params: the device tensor [B, N+1, np] the cut solve ran on; None = the resident tensor."""
        n = self._count(first, count)
        if params is None and first == 0 and n == self.B:
            self._chk(self.lib.sddp_continue_resident(self.h))
            return
        p = C.c_void_p(self.device_buffer(_lib.BUF_PARAMS)[0]) if params is None else self._dev(params, (self.B, self.N + 1, self.np_))
        self._chk(self.lib.sddp_continue_range_device(self.h, p, int(first), n))

    def unfinished(self, first: int = 0, count: int | None = None) -> int:
        """How many instances of [first, first + count) can be continued (waits for the stream)."""
        n = C.c_int()
        self._chk(self.lib.sddp_unfinished_count(self.h, int(first), self._count(first, count), C.byref(n)))
        return n.value

    def cut_and_continue(self, launch, *, total, first_slice=None, budget_us=None, min_iters=0, first=0, count=None, params=None,
                         between=None, drained=None, behind=None, keep_resume=False) -> int:
        """THE two-launch sequence of a solve that is cut and continued; it leaves the engine as it found it.  `launch()` enqueues a
        solve that covers the instances [first, first + count); it is cut at `first_slice` iterations or, at max_iters = total, after
        `budget_us` microseconds of device time with `min_iters` owed (exactly one of the two).  `between()` runs behind it; then
        the cut is lifted and, if any instance of the range is unfinished, a continue launch on `params` finishes those alone.
        `drained()` runs once the count is known (the stream has drained, the first launch's clocks still stand), `behind()` behind
        a continue launch.  -> the unfinished count: > 0 says that a second launch ran.
        Restored: max_iters; where resumable solves were on, the budget that was armed before; where they were off they go off
        again (which waits for the stream, frees the carry buffer and disarms any budget) unless keep_resume, the caller's
        persistent mode: they stay on, and are not touched if they were."""
        if (first_slice is None) == (budget_us is None):
            raise ValueError("exactly one of first_slice and budget_us cuts the first launch")
        nothing = lambda: None
        was_on, was_iters = self.resume_enabled, int(self.opts.max_iters)
        was_budget = self.time_budget() if was_on and budget_us is not None else None
        if not (was_on and keep_resume):
            self.enable_resume(True)                    # (nothing happens in the library when they are on)
        self.set_options(max_iters=int(total if first_slice is None else first_slice))
        if budget_us is not None:
            self.set_time_budget(budget_us, min_iters)
        launch()
        (between or nothing)()
        if budget_us is not None:
            self.set_time_budget(0.0)
        else:
            self.set_options(max_iters=int(total))
        n = self.unfinished(first, count)               # (waits for the stream)
        (drained or nothing)()
        if n > 0:
            self.continue_solve(params, first, count)
            (behind or nothing)()
        if not (was_on or keep_resume):
            self.enable_resume(False)
        elif was_budget is not None:
            self.set_time_budget(*was_budget)
        if int(self.opts.max_iters) != was_iters:
            self.set_options(max_iters=was_iters)
        return n

    # ---- time-budgeted launches: a launch that ends at a device-clock deadline, resumable (include/sddp.h) --------------------
    def set_time_budget(self, budget_us: float, min_iters: int = 0):
        """budget_us > 0: every later solve / continue launch of the handle ends `budget_us` microseconds of device time after its
        launch sequence started -- an instance still iterating then is left as a max_iters cut leaves it (status 1, resumable:
        continue_solve), the rest of the queue drains without iterating.  min_iters: the iterations every instance the launch runs
        is owed whatever the clock says (0: none, 1: the real-time-iteration setting).  budget_us = 0 disarms it.  Needs
        enable_resume() first; enable_resume(False) disarms it."""
        self._chk(self.lib.sddp_set_time_budget(self.h, float(budget_us), int(min_iters)))

    def time_budget(self):
        """-> (budget_us, min_iters) as armed; (0.0, 0): no budget."""
        b, m = C.c_double(), C.c_int()
        self._chk(self.lib.sddp_time_budget_info(self.h, C.byref(b), C.byref(m)))
        return b.value, m.value

    def deadline_clock(self):
        """(start, deadline) of the last launch sequence that ran under a budget, on the 100 MHz clock of slot_times() -- device
        buffer _lib.BUF_CLOCK; waits for the stream."""
        t = self._host_copy(_lib.BUF_CLOCK, "<i8").view(np.uint64)
        return int(t[0]), int(t[1])

    def deadline_overrun_us(self) -> float:
        """How far the last launch ran past its deadline, in microseconds: the latest slot end time (_lib.BUF_SLOT_TIMES) minus the
        deadline (_lib.BUF_CLOCK).  Negative: the launch was over that long before the deadline.  Meaningful only when the last
        solve / continue launch ran with a budget armed; waits for the stream."""
        _, deadline = self.deadline_clock()
        end = int(self.slot_times()[:, 1].max())
        return (end - deadline) / 100.0

    # ---- iteration log: one record per line search of every solve, kept on the device (include/sddp.h) ----------------------
    def enable_iteration_log(self, rows: int):
        """Every later solve launch keeps, per instance, one record of 16 doubles (_lib.LOG_FIELDS) per line search it ran, at most
        `rows` (1 .. 4096) of them; 0 frees the buffers.  Needs enable_resume() first (plain builds only)."""
        self._chk(self.lib.sddp_enable_iteration_log(self.h, int(rows)))

    def iteration_log_rows(self) -> int:
        """The rows per instance the log was enabled with (0: off)."""
        rows = C.c_int()
        self._chk(self.lib.sddp_iteration_log_info(self.h, C.byref(rows), None))
        return rows.value

    def iteration_log(self, first: int = 0, count: int | None = None):
        """-> (records [count, rows, 16], n [count] int32) of the instances [first, first + count) as numpy (waits for the stream):
        the rows [0, n[i]) of instance first + i are the line searches of its last solve, continue launches included."""
        n = self._count(first, count)
        rec = np.empty((max(n, 0), self.iteration_log_rows(), _lib.LOG_WORDS))
        cnt = np.empty(max(n, 0), dtype=np.int32)
        self._chk(self.lib.sddp_fetch_iteration_log(self.h, int(first), n, _lib.ptr(rec), _lib.ptr(cnt)))
        return rec, cnt

    def iteration_log_device(self):
        """Zero-copy torch views of the log in HBM: (records [B, rows, 16] float64, n [B] int32) -- the buffers _lib.BUF_LOG and BUF_LOG_COUNTS;
        ordered behind the handle's stream like fetch_device_views."""
        rows = self.device_buffer(_lib.BUF_LOG)[1] // (self.B * _lib.LOG_WORDS * 8)
        return self.device_view(_lib.BUF_LOG, (self.B, rows, _lib.LOG_WORDS)), self.device_view(_lib.BUF_LOG_COUNTS, (self.B,), "<i4")

    # ---- heterogeneous fleets: per-instance robot constants (include/sddp.h) ------------------------------------------------
    def set_instance_consts(self, overrides: dict, first: int = 0):
        """Instances [first, first + count) get their own robot: `overrides` maps a field of the model constants (m, I, com, feet,
        dt, force_scaling, the gains, lip_height, inertia_mode, lever_sign, relative_velocity_constraints) to an array
        [count, ...]; fields not named keep the handle's value.  From then on every kernel of the handle reads instance b's
        constants (solve on every entry point, queue keys, policy export, model_step, backward / forward); the other instances
        keep what they had -- the handle's constants, or an earlier override.  Unknown fields and fields that select a kernel
        build (barrier weights, bounds, user rows) raise ValueError before any GPU call."""
        rows = _lib.pack_instance_consts(self.consts, overrides)
        self._chk(self.lib.sddp_set_instance_consts(self.h, int(first), len(rows), rows))
        # (the packed rows as they went to the library, kept for const_gradient_fields: the chain rule needs each robot's own constants.
        #  The library has no call that reads a row back, so a table changed past this method is not seen here)
        self._instance_rows.append((int(first), rows))

    def clear_instance_consts(self):
        """Back to the handle's own constants for every instance."""
        self._chk(self.lib.sddp_clear_instance_consts(self.h))
        self._instance_rows.clear()

    def instance_consts_active(self) -> bool:
        on = C.c_int()
        self._chk(self.lib.sddp_instance_consts_active(self.h, C.byref(on)))
        return bool(on.value)

    # ---- class history (queue_order = 3) -------------------------------------------------------------------------------------
    def set_instance_classes(self, classes, n_classes: int):
        """classes [B] int (host): what kind of problem each instance is (-1: unlabelled); sddp.h queue_order 3.  Raises on a handle
        that labels its instances itself (enable_auto_classes)."""
        c = np.ascontiguousarray(classes, dtype=np.int32)
        if c.shape != (self.B,):
            raise ValueError(f"expected {self.B} class labels")
        self._chk(self.lib.sddp_set_instance_classes(self.h, _lib.ptr(c), int(n_classes)))

    def set_instance_classes_range_device(self, first: int, count: int, classes, n_classes: int):
        """labels of the instances [first, first + count) from a device int32 tensor (asynchronous on the handle's stream)"""
        import torch
        if not (isinstance(classes, torch.Tensor) and classes.is_cuda and classes.dtype == torch.int32 and classes.is_contiguous()
                and tuple(classes.shape) == (count,)):
            raise ValueError("expected a contiguous int32 CUDA tensor of `count` labels")
        self._chk(self.lib.sddp_set_instance_classes_range_device(self.h, int(first), int(count), C.c_void_p(classes.data_ptr()), int(n_classes)))

    def class_history(self, cls: int):
        """-> (mean iterations, solves) of class `cls` on this handle so far"""
        m, n = C.c_double(), C.c_longlong()
        self._chk(self.lib.sddp_class_history(self.h, int(cls), C.byref(m), C.byref(n)))
        return m.value, n.value

    # ---- auto classes: queue_order = 3 without caller labels; the history leaves and enters a handle (include/sddp.h) ---------------
    def enable_auto_classes(self, on: bool = True):
        """The handle labels its instances itself: every fresh solve launch computes, on the device and in front of everything else
        it launches, the label workload.schedule_classes(model, params) states -- stance pattern at node 0, nodes to the first
        contact switch, sign of the commanded velocity -- from the parameter tensor it runs on; n_classes = 36 (N + 2).  Raises if
        the caller set labels with another n_classes first; while on, set_instance_classes* raise.  on=False: the labelling
        stops, labels and history stay."""
        self._chk(self.lib.sddp_enable_auto_classes(self.h, int(bool(on))))

    def auto_classes_info(self):
        """-> (on, n_classes of the handle's class table whoever made it; 0: none)"""
        on, n = C.c_int(), C.c_int()
        self._chk(self.lib.sddp_auto_classes_info(self.h, C.byref(on), C.byref(n)))
        return bool(on.value), n.value

    def instance_classes(self, first: int = 0, count: int | None = None):
        """-> the class labels [count] int32 of the instances [first, first + count) (-1: unlabelled); waits for the stream."""
        n = self._count(first, count)
        out = np.empty(max(n, 0), dtype=np.int32)
        self._chk(self.lib.sddp_fetch_instance_classes(self.h, int(first), n, _lib.ptr(out)))
        return out

    def class_stats(self, first_class: int = 0, count: int | None = None):
        """-> the learned history [count, 2] uint64 = (sum of iterations, solves) of the classes [first_class, first_class + count),
        all of them by default; waits for the stream."""
        n = int(self.auto_classes_info()[1] - first_class if count is None else count)
        out = np.zeros((max(n, 0), 2), dtype=np.uint64)
        self._chk(self.lib.sddp_get_class_stats(self.h, int(first_class), n, _lib.ptr(out)))
        return out

    def add_class_stats(self, stats, first_class: int = 0):
        """ADD a history [count, 2] (class_stats() of another handle of the same N: a restarted server, another shard) to this
        handle's, classes [first_class, first_class + count); ordered on the handle's stream."""
        s = np.ascontiguousarray(stats, dtype=np.uint64)
        if s.ndim != 2 or s.shape[1] != 2:
            raise ValueError("expected stats of shape [count, 2]")
        self._chk(self.lib.sddp_add_class_stats(self.h, int(first_class), int(s.shape[0]), _lib.ptr(s)))

    RECORD_MODES = {"full": 0, "first_knot": 1, "first_knot_policy": 2}

    def record_words(self, mode="full"):
        w = C.c_int()
        self._chk(self.lib.sddp_record_words(self.h, self.RECORD_MODES[mode], C.byref(w)))
        return w.value

    def pack_records_device(self, out, first: int, count: int, mode="full"):
        """The solution records of the instances [first, first + count) into the device tensor `out` [count, record_words(mode)]
        (one kernel on the handle's stream, behind the solve): what a sharded fleet's all-gather sends."""
        self._chk(self.lib.sddp_pack_records_device(self.h, int(first), int(count), self.RECORD_MODES[mode],
                                                    self._dev(out, (count, self.record_words(mode)))))
        return out

    def last_queue_order(self):
        """Instance indices in the order the last queued launch handed them out (queue_order 1, 2 or 3); waits for the stream."""
        return self._host_copy(_lib.BUF_ORDER, "<i4")

    def slot_times(self):
        """[grid, 2] uint64: when each slot of the last solve launch started its first instance and when it found the queue empty
        (100 MHz constant-rate clock); waits for the stream."""
        return self._host_copy(_lib.BUF_SLOT_TIMES, "<i8").view(np.uint64).reshape(-1, 2)

    def queue_info(self):
        """(slots the work buffers exist for, grid of the last launch, queue length of the last launch or 0)."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.sddp_queue_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def poison_lds(self):
        """Diagnostic (include/sddp.h): fill the LDS of every CU with NaNs, so the next launch cannot pass on what an earlier kernel
        happened to leave in a word it reads before writing."""
        self._chk(self.lib.sddp_debug_poison_lds(self.h))

    def kernel_info(self):
        """-> dict(kernel, wavefronts_per_instance, waves_per_simd): the solve kernel the LAST launch of this handle ran
        (``solve_kernel[_w2]<model>`` on one wavefront per instance or ``solve_kernel_mw[_w2]<model>`` on four; ``_w2`` = the
        half-register-file build, which a handle asked for two per SIMD falls back from where it gains nothing)."""
        w, b, nm = C.c_int(), C.c_int(), C.c_char_p()
        self._chk(self.lib.sddp_kernel_info(self.h, C.byref(w), C.byref(b), C.byref(nm)))
        base = "solve_kernel_mw" if w.value == 4 else "solve_kernel"
        out = dict(kernel=f"{base}{'_w2' if b.value == 2 else ''}<{nm.value.decode()}>", wavefronts_per_instance=w.value,
                   waves_per_simd=b.value)
        v, sc, lds, per = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        if self.lib.sddp_kernel_resources(self.h, C.byref(v), C.byref(sc), C.byref(lds), C.byref(per)) == 0:
            out["resources"] = dict(vgprs=v.value, scratch_bytes_per_lane=sc.value, lds_bytes_per_workgroup=lds.value,
                                    workgroups_per_cu=per.value)
        return out


# ---- what the two single-robot adapters (ddp.DDPSolver, pyddp_hip.DdpSolver) share: an engine of batch 1 in the reference's layout ----
def default_warm_start(eng: DdpEngine, x0, have_x: bool, have_u: bool):
    """What the caller never set: x = x0 [1, nx] at every node, u = 0 (the examples pass no warm start; pyddp's default is unpinned)"""
    if not have_u:
        eng.set_u_warmstart(np.zeros((1, eng.N, eng.nu)))
    if not have_x:
        eng.set_x_warmstart(np.repeat(x0[:, None, :], eng.N + 1, axis=1))


def reference_layout(x, u, stats):
    """engine results x [1, N+1, nx], u [1, N, nu], stats [1] -> the reference's x [nx, N+1], u [nu, N], and the stats row"""
    return np.ascontiguousarray(x[0].T), np.ascontiguousarray(u[0].T), stats[0]


def eval_knots(model: str, N: int, k, x, u, p, consts: dict | None = None, model_id: int | None = None):
    """Per-knot model evaluation on the GPU: f, [fx fu], GN Hessian, gradient, cost (parity tests).  model_id: a user build."""
    lib = _lib.load()
    nx, nu, npar = _lib.model_dims(model)
    nz = nx + nu
    k = np.ascontiguousarray(k, dtype=np.int32)
    nk = k.shape[0]
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(nk, nx)
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(nk, nu)
    cst = _lib.default_consts(model, **(consts or {}))
    if cst.n_extra:
        npar += _lib.MAX_EXTRA               # the user rows' reference columns
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(nk, npar)
    f = np.empty((nk, nx)); F = np.empty((nk, nx, nz)); H = np.empty((nk, nz, nz)); g = np.empty((nk, nz)); L = np.empty(nk)
    _lib.check(lib.sddp_eval_knots(_lib.MODEL_IDS[model] if model_id is None else int(model_id), C.byref(cst), int(N), nk, _lib.ptr(k), _lib.ptr(x), _lib.ptr(u),
                                   _lib.ptr(p), _lib.ptr(f), _lib.ptr(F), _lib.ptr(H), _lib.ptr(g), _lib.ptr(L)))
    return f, F, H, g, L
