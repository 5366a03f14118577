"""User builds: non-linear (and linear) user residuals compiled into the SRBD device models.

A problem that declares a ``problem.NonlinearTerm`` gets a model build of its own.  This module

  * collects the problem's user rows -- LinearTerm and NonlinearTerm residuals in declaration order, at most 8 (``spec_from_problem``);
  * writes them as one C++ struct (``generate``): the row count NR, the structural non-zeros of de/dz as constexpr (row, col)
    tables, and ``eval(x, u, has_u, p, e, jv)`` -- the rows' values and, jv != nullptr, the non-zeros of their Jacobian, from
    ``sympy.cse`` + fp64 C expressions;
  * wraps the struct in a translation unit in the form of csrc/sddp_inst.hip that instantiates
    ``SrbdModel<..., kXrRows, struct>`` and exports extern "C" accessors (``source``);
  * compiles it for gfx950 into ``build/user/<key>.so`` (``ensure_build``), the key covering the source, the headers and the
    command line, so the same problem always finds the same build.

The library loads a build with ``sddp_register_user_build`` (include/sddp.h), which hands out a model id usable wherever a model id
is.  Gains, the constant parts of references and parameter values are runtime data: the weights live in the device table of the
"_x" builds (sddp_model_consts extra_*), the parameters the rows read in the parameter vector (the model's own columns and the 8
user columns behind them).  Changing them recompiles nothing.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .problem import LinearTerm, NonlinearTerm

# models with a user build: (number of the model's own parameters NPB, template arguments of SrbdModel before BAR)
MODELS = {"srbd13": (19, "2, false"), "srbd37": (19, "4, true")}
BASE_IDS = {"srbd13": 0, "srbd37": 1}
MAX_ROWS = 8
USER_DIR = os.path.join(_lib.ROOT, "build", "user")


@dataclass
class UserRow:
    kind: str                        # "state" (nodes 1..N) | "stage" (nodes 0..N-1)
    gain: float
    const: float = 0.0               # constant part of the reference (linear rows): runtime data, subtracted on the device
    a: np.ndarray | None = None      # linear row: coefficients over z = [x u]
    pcol: int | None = None          # linear row: index into the parameter vector of its reference, or None
    expr: object = None              # non-linear row: sympy expression over the symbols of `symmap`
    symmap: dict = field(default_factory=dict)   # symbol name -> ("x" | "u" | "p", index)


@dataclass
class UserSpec:
    model: str
    nx: int
    nu: int
    rows: list
    cols: list                       # user parameter columns: (Parameter, row) per column NPB + j

    def extra_rows(self):
        """sddp_model_consts extra_* of the build: weights, kinds, constant parts (the coefficients are compiled in)."""
        return [dict(a=np.zeros(self.nx + self.nu), w=r.gain, kind=r.kind, const=r.const) for r in self.rows]


def spec_from_problem(prb, nx: int, nu: int) -> UserSpec | None:
    """The user rows of a problem (LinearTerm and NonlinearTerm residuals in declaration order), or None when it declares no
    NonlinearTerm.  Raises NotImplementedError for what a user build cannot express."""
    cost = prb.function_container.getCost()
    if not any(isinstance(fn.term, NonlinearTerm) for fn in cost.values()):
        return None
    if prb.model not in MODELS:
        raise NotImplementedError(f"non-linear residuals are implemented for srbd13 and srbd37 only (model {prb.model})")
    npb = MODELS[prb.model][0]
    ns = prb.nodes - 1
    ranges = {"state": list(range(1, ns + 1)), "stage": list(range(0, ns))}
    symmap, off = {}, {}
    o = 0
    for v in list(prb.getState().getVars()) + list(prb.getInput().getVars()):
        off[v] = o
        for i in range(v.getDim()):
            symmap[f"{v.getName()}_{i}"] = ("x", o + i) if o + i < nx else ("u", o + i - nx)
        o += v.getDim()
    own, user_pars = 0, []
    for p in prb.getParameters().values():
        if own < npb:
            for i in range(p.getDim()):
                symmap[f"{p.getName()}_{i}"] = ("p", own + i)
            own += p.getDim()
        else:
            user_pars.append(p)
    cols, rows = [], []

    def col_of(par, r):
        for j, (q, rr) in enumerate(cols):
            if q is par and rr == r:
                return npb + j
        cols.append((par, r))
        return npb + len(cols) - 1

    for name, fn in cost.items():
        t = fn.term
        if not isinstance(t, (LinearTerm, NonlinearTerm)):
            continue
        nodes = fn.getNodes()
        kind = "state" if nodes == ranges["state"] else ("stage" if nodes == ranges["stage"] else None)
        if kind is None:
            raise NotImplementedError(f"residual {name!r}: a user residual lives on nodes 1..N (state term) or 0..N-1 (stage term)")
        if isinstance(t, LinearTerm):
            for r in range(t.dim):
                a = np.zeros(nx + nu)
                for v, A in t.coeffs.items():
                    if v not in off:
                        raise ValueError(f"residual {name!r}: {v} is not a state or input variable of this problem")
                    a[off[v]:off[v] + v.getDim()] += A[r]
                if kind == "state" and np.any(a[nx:] != 0.0):
                    raise NotImplementedError(f"residual {name!r}: a term on nodes 1..N is active at the terminal node and cannot touch the inputs")
                rows.append(UserRow(kind, t.gain, float(t.const[r]), a=a, pcol=None if t.ref is None else col_of(t.ref, r)))
            continue
        local = {}
        for r, e in enumerate(t.exprs):
            for s in sorted(e.free_symbols, key=lambda s: s.name):
                if s.name in symmap:
                    ent = symmap[s.name]
                else:                                               # a user parameter: one of the 8 user columns
                    par = next((p for p in user_pars if s.name.startswith(p.getName() + "_")
                                and s.name[len(p.getName()) + 1:].isdigit() and int(s.name[len(p.getName()) + 1:]) < p.getDim()), None)
                    if par is None:
                        raise ValueError(f"residual {name!r}: symbol {s.name} belongs to no variable or parameter of this problem")
                    ent = ("p", col_of(par, int(s.name[len(par.getName()) + 1:])))
                if kind == "state" and ent[0] == "u":
                    raise NotImplementedError(f"residual {name!r}: a term on nodes 1..N is active at the terminal node and cannot read "
                                              f"the inputs ({s.name})")
                local[s.name] = ent
            rows.append(UserRow(kind, t.gain, 0.0, expr=e, symmap=dict(local)))
    if len(rows) > MAX_ROWS:
        raise NotImplementedError(f"{len(rows)} user residual rows declared; the models carry at most {MAX_ROWS}")
    if len(cols) > MAX_ROWS:
        raise NotImplementedError(f"the user residuals read {len(cols)} user parameter entries; the models carry at most {MAX_ROWS}")
    return UserSpec(prb.model, nx, nu, rows, cols)


# ---- code generation ----------------------------------------------------------------------------------------------------------
def _printer():
    from sympy.printing.c import C99CodePrinter

    class Printer(C99CodePrinter):
        """fp64 C: doubles printed round-trip exact, small integer powers as products, constants as literals."""

        def _print_Float(self, e):
            return repr(float(e))

        def _print_Rational(self, e):
            return f"({float(e.p)!r} / {float(e.q)!r})"

        def _print_Integer(self, e):
            return repr(float(int(e)))

        def _print_NumberSymbol(self, e):
            return repr(float(e))

        _print_Pi = _print_Exp1 = _print_NumberSymbol

        def _print_Pow(self, e):
            b, x = self._print(e.base), e.exp
            if x.is_Integer and 1 <= abs(int(x)) <= 4:
                prod = "*".join([f"({b})"] * abs(int(x)))
                return f"({prod})" if int(x) > 0 else f"(1.0 / ({prod}))"
            if x == 0.5:
                return f"sqrt({b})"
            if x == -0.5:
                return f"(1.0 / sqrt({b}))"
            return f"pow({b}, {repr(float(x))})"

    return Printer()


def _z_name(ent):
    kind, i = ent
    return {"x": f"x[{i}]", "u": f"u[{i}]", "p": f"p[{i}]"}[kind]


def _z_index(ent, nx):
    return ent[1] if ent[0] == "x" else (nx + ent[1] if ent[0] == "u" else None)


def _row_exprs(spec: UserSpec, j: int):
    """Row j as (value expression, [(z column, derivative expression)]) over symbols named by their C access (x[i], u[i], p[i])."""
    import sympy
    r = spec.rows[j]
    if r.expr is None:                                        # linear row: a . z - p_ref
        terms, jac = [], []
        for i in np.nonzero(r.a)[0]:
            zi = sympy.Symbol(f"x[{i}]" if i < spec.nx else f"u[{i - spec.nx}]", real=True)
            c = sympy.Float(float(r.a[i]), 17)
            terms.append(c * zi)
            jac.append((int(i), c))
        e = sympy.Add(*terms)
        if r.pcol is not None:
            e = e - sympy.Symbol(f"p[{r.pcol}]", real=True)
        return e, jac
    sub = {sympy.Symbol(n, real=True): sympy.Symbol(_z_name(ent), real=True) for n, ent in r.symmap.items()}
    e = r.expr.xreplace(sub)
    jac = []
    for n, ent in sorted(r.symmap.items(), key=lambda t: (t[1][0] == "p", _z_index(t[1], spec.nx) or 0)):
        zi = _z_index(ent, spec.nx)
        if zi is None:
            continue
        d = sympy.diff(e, sympy.Symbol(_z_name(ent), real=True))
        if d != 0:
            jac.append((zi, d))
    jac.sort(key=lambda t: t[0])
    return e, jac


def _block(pr, vals, jacs, ind, with_jac):
    """C statements for the value expressions vals [(row, expr)] and, with_jac, the Jacobian entries jacs [(n, expr)].  One
    sympy.cse over values and Jacobian; the value-only block keeps the temporaries its values need, so both blocks compute
    bit-identical values."""
    import sympy
    exprs = [e for _, e in vals] + [e for _, e in jacs]
    if not exprs:
        return []
    subs, red = sympy.cse(exprs, symbols=sympy.numbered_symbols("t"), order="canonical")
    outs = red if with_jac else red[:len(vals)]
    need = set().union(*[e.free_symbols for e in outs]) if outs else set()
    keep = []
    for sym, val in reversed(subs):
        if sym in need:
            keep.append((sym, val))
            need |= val.free_symbols
    out = [f"{ind}const double {pr._print(sym)} = {pr._print(val)};" for sym, val in reversed(keep)]
    for (j, _), e in zip(vals, red[:len(vals)]):
        out.append(f"{ind}e[{j}] = {pr._print(e)};")
    if with_jac:
        for (n, _), e in zip(jacs, red[len(vals):]):
            out.append(f"{ind}jv[{n}] = {pr._print(e)};")
    return out


def generate(spec: UserSpec) -> str:
    """The C++ struct of the spec's user rows (deterministic for one spec).  Compiles as HIP device code and as host C++."""
    pr = _printer()
    nr = len(spec.rows)
    per_row = [_row_exprs(spec, j) for j in range(nr)]
    rows, cols, ent = [], [], {}
    for j, (_, jac) in enumerate(per_row):
        for zi, d in jac:
            ent[(j, len(rows))] = d
            rows.append(j)
            cols.append(zi)
    nnz = len(rows)
    if nnz == 0:
        raise ValueError("user residuals: no row depends on a state or input")
    body = []
    for kind, guard in (("state", None), ("stage", "has_u")):
        idx = [j for j in range(nr) if spec.rows[j].kind == kind]
        if not idx:
            continue
        vals = [(j, per_row[j][0]) for j in idx]
        jacs = [(n, ent[(rows[n], n)]) for n in range(nnz) if rows[n] in idx]
        o = " " * (8 if guard is None else 12)
        blk = ([f"{o}if (jv) {{"] + _block(pr, vals, jacs, o + "    ", True) + [f"{o}}} else {{"] + _block(pr, vals, jacs, o + "    ", False)
               + [f"{o}}}"])
        if guard is None:
            body += blk
        else:                          # the terminal node (has_u false): the stage rows are 0 and no input is read
            zero = [f"            e[{j}] = 0.0;" for j in idx] + ["            if (jv) {"] + [f"                jv[{n}] = 0.0;" for n, _ in jacs] + ["            }"]
            body += ["        if (has_u) {"] + blk + ["        } else {"] + zero + ["        }"]

    def chain(t):
        return " : ".join(f"n == {n} ? {v}" for n, v in enumerate(t[:-1])) + (" : " if len(t) > 1 else "") + str(t[-1])

    kinds = ", ".join("0" if r.kind == "state" else "1" for r in spec.rows)
    text = "\n".join([
        f"// user rows of a {spec.model} user build: {nr} rows, {nnz} structural non-zeros of de/dz (z = [x u]).",
        "// Generated by srbd_horizon_amd/userterms.py.",
        "struct SddpUserRows {",
        f"    static constexpr int NR = {nr}, NNZ = {nnz};",
        f"    static constexpr int KIND[NR] = {{{kinds}}};      // 0: state row (nodes 1..N), 1: stage row (nodes 0..N-1)",
        f"    static constexpr int ROWS[NNZ] = {{{', '.join(map(str, rows))}}};",
        f"    static constexpr int COLS[NNZ] = {{{', '.join(map(str, cols))}}};",
        f"    SDDP_UR_HD static constexpr int row(int n) {{ return {chain(rows)}; }}",
        f"    SDDP_UR_HD static constexpr int col(int n) {{ return {chain(cols)}; }}",
        "    // e[NR]: the rows' values; jv[NNZ] (or nullptr): the Jacobian's non-zeros.  has_u false: the stage rows are 0, u is not read",
        "    template <class XV, class UV>",
        "    SDDP_UR_HD static inline __attribute__((always_inline)) void eval(XV x, UV u, bool has_u, const double* p, double* e, double* jv) {",
        "        (void)x; (void)u; (void)has_u; (void)p;",
        *body,
        "    }",
        "};",
        ""])
    return text


HOST_PRELUDE = """#include <cmath>
#if defined(__HIPCC__) || defined(__HIP__)
#define SDDP_UR_HD __host__ __device__
#else
#define SDDP_UR_HD
#endif
using std::sqrt; using std::pow; using std::exp; using std::log; using std::sin; using std::cos; using std::tan; using std::tanh; using std::atan;
"""


def source(spec: UserSpec) -> str:
    """The translation unit of a user build (the form of csrc/sddp_inst.hip).  One unit, one shared object: it is the build's main
    unit and its inspect unit at once, and defines side_inspect_ops for its model, with csrc/sddp_inst.hip's own macro, in front of the
    make_ops that enters it."""
    npb, targs = MODELS[spec.model]
    mw_check = ("static_assert(!use_mw<SddpUserModel>(), \"srbd13's user build stays on the one-wave kernel (LDS under the 48 KB switch)\");"
                if spec.model == "srbd13" else "")
    return f"""// user build of {spec.model} -- generated by srbd_horizon_amd/userterms.py; loaded by sddp_register_user_build (include/sddp.h)
#include "sddp_launch.hpp"
#include "sddp_launch_inspect.hpp"

{HOST_PRELUDE}
{generate(spec)}
namespace sddp {{
using SddpUserModel = SrbdModel<{targs}, false, false, kXrRows, ::SddpUserRows>;
static_assert(SddpUserModel::NPB == {npb}, "parameter layout of the generated rows");
{mw_check}
SDDP_DEFINE_INSPECT_OPS(SddpUserModel)
}}  // namespace sddp

#define SDDP_USER_EXPORT extern "C" __attribute__((visibility("default")))
SDDP_USER_EXPORT const sddp::ModelOps* sddp_user_ops() {{
    static const sddp::ModelOps ops = sddp::make_ops<sddp::SddpUserModel>("{spec.model}");
    return &ops;
}}
SDDP_USER_EXPORT int sddp_user_base_model() {{ return {BASE_IDS[spec.model]}; }}
SDDP_USER_EXPORT unsigned long long sddp_user_header_stamp() {{ return SDDP_HEADER_STAMP; }}
SDDP_USER_EXPORT int sddp_user_rows() {{ return {len(spec.rows)}; }}
"""


# ---- compilation ------------------------------------------------------------------------------------------------------------
def _command(src_path: str, out_path: str, root: str = _lib.ROOT):
    """A user build is compiled like a model build of the library (_lib.compile_command); the tail is its own: one shared object of
    the generated unit, which exports the accessors alone."""
    return _lib.compile_command(root=root) + ["-fvisibility=hidden", f"-DSDDP_HEADER_STAMP={_lib.header_stamp(root)}ULL", "-shared", src_path,
                                              "-o", out_path]


def build_key(src: str, root: str = _lib.ROOT) -> str:
    """Cache key of a user build: the generated source, csrc/*.hpp, include/sddp.h and the command line
    (paths relative to the tree, so a tree built elsewhere finds its builds)."""
    h = hashlib.sha256(src.encode())
    csrc = os.path.join(root, "srbd_horizon_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hpp"):
            h.update(f.encode())
            h.update(open(os.path.join(csrc, f), "rb").read())
    h.update(open(os.path.join(root, "include", "sddp.h"), "rb").read())
    h.update(" ".join(_command("<src>", "<out>", root)).replace(root, "<root>").encode())
    return h.hexdigest()[:20]


def build_path(spec: UserSpec) -> str:
    return os.path.join(USER_DIR, build_key(source(spec)) + ".so")


def ensure_build(spec: UserSpec, verbose: bool = False) -> str:
    """Path of the spec's user build; compiled here when missing (needs hipcc), else an error naming the build and build()."""
    src = source(spec)
    key = build_key(src)
    out = os.path.join(USER_DIR, key + ".so")
    if os.path.exists(out):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        raise RuntimeError(f"user build {out} is missing and there is no hipcc to compile it: build it beforehand "
                           "(__graft_entry__.build() pre-builds the tests' and the example's user builds)")
    os.makedirs(USER_DIR, exist_ok=True)
    src_path = os.path.join(USER_DIR, key + ".hip")
    with open(src_path, "w") as f:
        f.write(src)
    tmp = out + f".tmp{os.getpid()}"
    cmd = _command(src_path, tmp)
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(tmp, out)
    return out


_registered = {}


def register(spec: UserSpec) -> int:
    """Build (if needed) and register the spec's user build with the library; returns its model id (>= 16)."""
    import ctypes as C
    path = ensure_build(spec)
    if path not in _registered:
        mid = C.c_int()
        _lib.check(_lib.load().sddp_register_user_build(path.encode(), C.byref(mid)))
        _registered[path] = mid.value
    return _registered[path]
