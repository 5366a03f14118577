"""Test-side oracle of the user builds: a numpy model (oracle/models.py) plus the user rows of a userterms.UserSpec, evaluated
through sympy.lambdify -- in the style of oracle/models.py WithLinearRows: the parameter vector is 8 columns wider, the dynamics
are the base model's."""
from __future__ import annotations

import numpy as np

from oracle import models as omodels

NXR = 8


class WithUserRows(omodels.Model):
    def __init__(self, base: omodels.Model, spec):
        import sympy
        self.base, self.cst, self.spec = base, base.cst, spec
        self.name = base.name
        self.nx, self.nu, self.npb = base.nx, base.nu, base.np_
        self.np_ = base.np_ + NXR
        self._fns = []
        for r in spec.rows:
            if r.expr is None:
                self._fns.append(None)
                continue
            names = sorted(r.symmap)
            syms = [sympy.Symbol(n, real=True) for n in names]
            grads = []
            for n, s in zip(names, syms):
                kind, i = r.symmap[n]
                if kind != "p":
                    grads.append((i if kind == "x" else self.nx + i, sympy.lambdify(syms, sympy.diff(r.expr, s), "math")))
            self._fns.append(([r.symmap[n] for n in names], sympy.lambdify(syms, r.expr, "math"), grads))

    def _row(self, j, x, u, p):
        """value and gradient over z of user row j (u None: the terminal node)"""
        r = self.spec.rows[j]
        z = np.concatenate([x, u if u is not None else np.zeros(self.nu)])
        if r.expr is None:
            return float(r.a @ z) - (p[r.pcol] if r.pcol is not None else 0.0) - r.const, np.asarray(r.a, dtype=float)
        ents, fe, grads = self._fns[j]
        vals = [x[i] if k == "x" else (u[i] if k == "u" else p[i]) for k, i in ents]
        J = np.zeros(self.nx + self.nu)
        for zi, fg in grads:
            J[zi] += fg(*vals)
        return fe(*vals) - r.const, J

    def f(self, x, u, p):
        return self.base.f(x, u, p[:self.npb])

    def f_jac(self, x, u, p):
        return self.base.f_jac(x, u, p[:self.npb])

    def residual_jac(self, x, u, p, k):
        r, Jx, Ju = self.base.residual_jac(x, u, p[:self.npb], k)
        rr, jx, ju = [r], [Jx], [Ju]
        for j, row in enumerate(self.spec.rows):
            active = (k >= 1) if row.kind == "state" else (u is not None)
            if not active:
                continue
            e, J = self._row(j, x, u, p)
            g = np.sqrt(row.gain)
            rr.append(np.array([g * e]))
            jx.append(g * J[None, :self.nx]); ju.append(g * J[None, self.nx:])
        return np.concatenate(rr), np.vstack(jx), np.vstack(ju)

    def second_order_ux(self, x, u, p, vp):
        return self.base.second_order_ux(x, u, p[:self.npb], vp)

    def initial_state(self):
        return self.base.initial_state()

    def static_input(self):
        return self.base.static_input()
