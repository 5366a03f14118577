"""User residuals compiled into the SRBD device models (srbd_horizon_amd/userterms.py), without a GPU: the generated code against
sympy, what NonlinearTerm and the adapter refuse, the cache key, and a user build compiled for gfx950."""
import ctypes.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sympy = pytest.importorskip("sympy")

from srbd_horizon_amd import _lib, userterms  # noqa: E402
from srbd_horizon_amd.ddp import DDPSolver  # noqa: E402
from srbd_horizon_amd.prb import LIPProblem, SRBD13Problem, SRBDProblem  # noqa: E402
from srbd_horizon_amd.problem import NonlinearTerm  # noqa: E402
from tests import user_terms_defs as defs  # noqa: E402

ROOT = _lib.ROOT


def _var(prb):
    return {v.getName(): v for v in prb.var_container.getVarList(offset=False)}


def kitchen_sink(ns=10):
    """srbd13 with every allowed function in one state term and one stage term."""
    pb = SRBD13Problem()
    prb = pb.createSRBD13Problem(ns, 1.0)
    v = _var(prb)
    r, o, rd, w, f0, f1 = (v[n].sym() for n in ("r", "o", "rdot", "w", "f0", "f1"))
    q = prb.createParameter("q", 2)
    e_state = [sympy.exp(0.1 * r[0]) + sympy.log(2 + r[1] ** 2) + sympy.sqrt(1 + rd[0] ** 2) + sympy.tan(0.1 * w[0]),
               sympy.atan(w[1]) * sympy.tanh(o[0]) + r[2] ** 3 - q.sym()[0] / (1 + o[1] ** 2) + (1 + r[0] ** 2) ** 1.5
               + sympy.cos(o[2]) * sympy.sin(o[3]) + sympy.pi * rd[2] ** -2 + sympy.Rational(1, 3) * q.sym()[1]]
    e_stage = [f0[2] * f1[2] / 1000 + sympy.sqrt(2 + f0[0] ** 2) - r[0] * f1[1], 1 / sympy.sqrt(3 + f1[0] ** 2)]
    prb.createResidual("sink_state", NonlinearTerm(sympy.Matrix(e_state), gain=2.0), nodes=range(1, ns + 1))
    prb.createResidual("sink_stage", NonlinearTerm(e_stage, gain=0.5), nodes=range(0, ns))
    return pb, prb


def _host_eval(spec, X, U, P, has_u=True):
    """Compile the generated struct as host C++ (g++) and evaluate it at the points: (e [n, NR], J [n, NR, nz] scattered)."""
    nr = len(spec.rows)
    src = userterms.HOST_PRELUDE + userterms.generate(spec) + r"""
#include <cstdio>
#include <vector>
int main(int argc, char** argv) {
    const int n = std::atoi(argv[1]), nx = std::atoi(argv[2]), nu = std::atoi(argv[3]), np_ = std::atoi(argv[4]), has_u = std::atoi(argv[5]);
    std::vector<double> x(nx), u(nu), p(np_), e(SddpUserRows::NR), jv(SddpUserRows::NNZ);
    FILE* in = std::fopen(argv[6], "rb");
    FILE* out = std::fopen(argv[7], "wb");
    for (int n0 = 0; n0 < SddpUserRows::NNZ; ++n0) { double a = SddpUserRows::ROWS[n0], b = SddpUserRows::COLS[n0];
        std::fwrite(&a, 8, 1, out); std::fwrite(&b, 8, 1, out); }
    for (int i = 0; i < n; ++i) {
        if (std::fread(x.data(), 8, nx, in) != size_t(nx) || std::fread(u.data(), 8, nu, in) != size_t(nu) || std::fread(p.data(), 8, np_, in) != size_t(np_)) return 2;
        SddpUserRows::eval(x.data(), has_u ? u.data() : x.data(), has_u != 0, p.data(), e.data(), jv.data());
        std::fwrite(e.data(), 8, e.size(), out);
        std::fwrite(jv.data(), 8, jv.size(), out);
        SddpUserRows::eval(x.data(), has_u ? u.data() : x.data(), has_u != 0, p.data(), e.data(), (double*)nullptr);   // value-only path
        std::fwrite(e.data(), 8, e.size(), out);
    }
    std::fclose(out);
    return 0;
}
"""
    d = tempfile.mkdtemp()
    try:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(src.replace("#include <cstdio>", "#include <cstdio>\n#include <cstdlib>"))
        subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(d, "t.cpp"), "-o", os.path.join(d, "t")], check=True)
        n = X.shape[0]
        np.concatenate([X, U, P], axis=1).astype(np.float64).tofile(os.path.join(d, "in.bin"))
        subprocess.run([os.path.join(d, "t"), str(n), str(X.shape[1]), str(U.shape[1]), str(P.shape[1]), str(int(has_u)),
                        os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], check=True)
        raw = np.fromfile(os.path.join(d, "out.bin"))
    finally:
        shutil.rmtree(d)
    # header: NNZ (row, col) pairs, then per point e [NR] | jv [NNZ] | e again (value-only path)
    nnz = next(k for k in range(0, 129) if (raw.size - 2 * k) == n * (2 * nr + k))
    rc = raw[:2 * nnz].reshape(nnz, 2).astype(int)
    body = raw[2 * nnz:].reshape(n, 2 * nr + nnz)
    e, jv, e2 = body[:, :nr], body[:, nr:nr + nnz], body[:, nr + nnz:]
    J = np.zeros((n, nr, spec.nx + spec.nu))
    for t, (row, col) in enumerate(rc):
        J[:, row, col] += jv[:, t]
    return e, J, e2


def _sympy_eval(spec, X, U, P):
    """The rows and their Jacobians through sympy.lambdify of the user's own expressions."""
    n, nz = X.shape[0], spec.nx + spec.nu
    E = np.zeros((n, len(spec.rows)))
    J = np.zeros((n, len(spec.rows), nz))
    Z = np.concatenate([X, U], axis=1)
    for j, r in enumerate(spec.rows):
        if r.expr is None:
            E[:, j] = Z @ r.a - (P[:, r.pcol] if r.pcol is not None else 0.0)
            J[:, j, :] = r.a
            continue
        names = sorted(r.symmap)
        syms = [sympy.Symbol(s, real=True) for s in names]
        cols = [(X if r.symmap[s][0] == "x" else (U if r.symmap[s][0] == "u" else P))[:, r.symmap[s][1]] for s in names]
        E[:, j] = np.broadcast_to(sympy.lambdify(syms, r.expr, "numpy")(*cols), (n,))
        for s, sy in zip(names, syms):
            kind, i = r.symmap[s]
            if kind == "p":
                continue
            zi = i if kind == "x" else spec.nx + i
            J[:, j, zi] += np.broadcast_to(sympy.lambdify(syms, sympy.diff(r.expr, sy), "numpy")(*cols), (n,))
    return E, J


CASES = {
    "srbd13_terrain": lambda: defs.srbd13_terrain(10)[1],
    "srbd13_pair_nonlinear": lambda: defs.srbd13_pair(10, True)[1],
    "srbd37_reach": lambda: defs.srbd37_reach(10)[1],
    "srbd13_kitchen_sink": lambda: kitchen_sink()[1],
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_generated_eval_matches_sympy(case):
    spec = defs.spec_of(CASES[case]())
    rng = np.random.default_rng(7)
    n = 200
    X = rng.uniform(-1.0, 1.0, (n, spec.nx))
    U = rng.uniform(-1.0, 1.0, (n, spec.nu)) * 50.0
    P = rng.uniform(0.5, 1.5, (n, 19 + 8))
    e, J, e2 = _host_eval(spec, X, U, P)
    E, JS = _sympy_eval(spec, X, U, P)
    np.testing.assert_allclose(e, E, rtol=1e-13, atol=1e-13 * np.abs(E).max())
    np.testing.assert_allclose(J, JS, rtol=1e-13, atol=1e-13 * max(np.abs(JS).max(), 1.0))
    np.testing.assert_array_equal(e2, e)                                      # the value-only path computes the same values
    # the terminal node (has_u false): stage rows 0 with a zero Jacobian, state rows unchanged
    e0, J0, _ = _host_eval(spec, X[:8], U[:8], P[:8], has_u=False)
    for j, r in enumerate(spec.rows):
        if r.kind == "stage":
            assert np.all(e0[:, j] == 0.0) and np.all(J0[:, j] == 0.0)
        else:
            np.testing.assert_array_equal(e0[:, j], e[:8, j])


@pytest.mark.parametrize("bad", ["Piecewise", "Abs", "Max", "Min", "sign", "atan2", "symbolic_power", "alien", "nan"])
def test_refused_functions(bad):
    prb = SRBD13Problem().createSRBD13Problem(5, 1.0)
    r = _var(prb)["r"].sym()
    expr = {"Piecewise": sympy.Piecewise((r[0], r[1] > 0), (r[1], True)), "Abs": sympy.Abs(r[0]), "Max": sympy.Max(r[0], r[1]),
            "Min": sympy.Min(r[0], r[1]), "sign": sympy.sign(r[0]), "atan2": sympy.atan2(r[0], r[1]), "symbolic_power": r[0] ** r[1],
            "alien": r[0] + sympy.Symbol("not_a_variable"), "nan": r[0] + sympy.nan}[bad]
    with pytest.raises(ValueError, match="."):
        NonlinearTerm(expr, gain=1.0)


@pytest.mark.parametrize("gain", [-1.0, float("inf"), float("nan")])
def test_refused_gain(gain):
    prb = SRBD13Problem().createSRBD13Problem(5, 1.0)
    with pytest.raises(ValueError, match="gain"):
        NonlinearTerm(_var(prb)["r"].sym()[0], gain=gain)


def test_symbol_of_another_problem_is_refused():
    a = SRBD13Problem().createSRBD13Problem(5, 1.0)
    b = SRBDProblem().createSRBDProblem(5, 1.0)
    e = _var(b)["cdot0"].sym()[0]                                # a state of the srbd37 problem: no such entry in srbd13
    with pytest.raises(ValueError, match="belong to no variable"):
        a.createResidual("alien", NonlinearTerm(e, gain=1.0), nodes=range(1, 6))


def _solver_error(prb, opts=None, exc=NotImplementedError, match="."):
    with pytest.raises(exc, match=match):
        DDPSolver(prb, opts or {})


def test_refused_shapes():
    ns = 5
    # a state term (nodes 1..N) that reads an input
    prb = SRBD13Problem().createSRBD13Problem(ns, 1.0)
    v = _var(prb)
    prb.createResidual("bad", NonlinearTerm(v["r"].sym()[0] * v["f0"].sym()[2], gain=1.0), nodes=range(1, ns + 1))
    _solver_error(prb, match="cannot read the inputs")
    # more than 8 rows
    prb = SRBD13Problem().createSRBD13Problem(ns, 1.0)
    x = sympy.Matrix(list(_var(prb)["r"].sym()) + list(_var(prb)["rdot"].sym()) + list(_var(prb)["w"].sym()))
    prb.createResidual("many", NonlinearTerm(x.applyfunc(lambda s: s ** 2), gain=1.0), nodes=range(1, ns + 1))
    _solver_error(prb, match="at most 8")
    # node ranges other than 1..N / 0..N-1
    prb = SRBD13Problem().createSRBD13Problem(ns, 1.0)
    prb.createResidual("odd", NonlinearTerm(_var(prb)["r"].sym()[0] ** 2, gain=1.0), nodes=range(2, ns + 1))
    _solver_error(prb, match="nodes 1..N")
    # lip30 and srbd61
    lp = LIPProblem()
    prb = lp.createLIPProblem(ns, 1.0)
    prb.createResidual("r2", NonlinearTerm(_var(prb)["r"].sym()[0] ** 2, gain=1.0), nodes=range(1, ns + 1))
    _solver_error(prb, match="srbd13 and srbd37 only")
    prb = SRBDProblem().createSRBDProblem(ns, 1.0, params={"contact_model": 4})
    assert prb.model == "srbd61"
    prb.createResidual("r2", NonlinearTerm(_var(prb)["r"].sym()[0] ** 2, gain=1.0), nodes=range(1, ns + 1))
    _solver_error(prb, match="srbd13 and srbd37 only")
    # a barrier, second_order = 2
    for opts, match in (({"bound_barrier_weight": 1.0}, "no barrier"), ({"second_order": 2}, "second_order = 2")):
        prb = SRBD13Problem().createSRBD13Problem(ns, 1.0)
        prb.createResidual("r2", NonlinearTerm(_var(prb)["r"].sym()[0] ** 2, gain=1.0), nodes=range(1, ns + 1))
        _solver_error(prb, opts, match=match)


def test_generated_text_is_deterministic():
    code = ("import sys; sys.path.insert(0, %r); from tests import user_terms_defs as d; from srbd_horizon_amd import userterms as u; "
            "print(u.source(d.spec_of(d.srbd37_reach(20)[1])))" % ROOT)
    outs = {subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True,
                           env={**os.environ, "PYTHONHASHSEED": str(seed)}).stdout for seed in (1, 2)}
    assert len(outs) == 1
    assert userterms.source(defs.spec_of(defs.srbd37_reach(20)[1])) == outs.pop().rstrip("\n") + "\n"


def test_gains_and_values_are_runtime_data():
    a = defs.spec_of(defs.srbd13_terrain(20, a=0.03, gain=1e3)[1])
    b = defs.spec_of(defs.srbd13_terrain(20, a=0.07, k=3.0, gain=5.0)[1])
    assert userterms.source(a) == userterms.source(b)
    assert [r["w"] for r in b.extra_rows()] == [5.0]


def test_cache_key_covers_the_headers():
    src = userterms.source(defs.spec_of(defs.srbd13_terrain(20)[1]))
    d = tempfile.mkdtemp()
    try:
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(d, "include"))
        shutil.copytree(os.path.join(ROOT, "srbd_horizon_amd", "csrc"), os.path.join(d, "srbd_horizon_amd", "csrc"))
        k0 = userterms.build_key(src, root=d)
        assert k0 == userterms.build_key(src, root=ROOT)           # relative to the tree: the same key wherever it is built
        for h in ("srbd_horizon_amd/csrc/sddp_models.hpp", "include/sddp.h"):
            with open(os.path.join(d, h), "a") as f:
                f.write("\n// changed\n")
            k1 = userterms.build_key(src, root=d)
            assert k1 != k0
            k0 = k1
        assert userterms.build_key(src + "\n", root=d) != k0
    finally:
        shutil.rmtree(d)


def test_missing_build_without_compiler_names_build(monkeypatch, tmp_path):
    monkeypatch.setattr(userterms, "USER_DIR", str(tmp_path))
    monkeypatch.setenv("HIPCC", str(tmp_path / "no-hipcc"))
    with pytest.raises(RuntimeError, match=r"build\(\)"):
        userterms.ensure_build(defs.spec_of(defs.srbd13_terrain(20)[1]))


def _dynamic_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}


def test_user_build_compiles_for_gfx950_and_is_self_contained():
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    spec = defs.spec_of(defs.srbd13_terrain(20)[1])
    path = userterms.ensure_build(spec)
    assert os.path.basename(path) == userterms.build_key(userterms.source(spec)) + ".so"
    exported = _dynamic_symbols(path)
    for acc in ("sddp_user_ops", "sddp_user_base_model", "sddp_user_header_stamp", "sddp_user_rows"):
        assert acc in exported
    assert not any(s.startswith("sddp_") and not s.startswith("sddp_user_") for s in exported)
    # gfx950 device code inside
    bundles = subprocess.run(["/opt/rocm/llvm/bin/clang-offload-bundler", "--list", "--type=o", "--input=" + path],
                             capture_output=True, text=True)
    assert "gfx950" in bundles.stdout or b"gfx950" in open(path, "rb").read()
    # every undefined symbol is provided by the HIP runtime, libc, libm, libgcc or libstdc++
    out = subprocess.run(["nm", "-D", "--undefined-only", path], check=True, capture_output=True, text=True).stdout
    undef = {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip() and ln.split()[0] == "U"}
    provided = set()
    for name in ("amdhip64", "c", "m", "gcc_s", "stdc++"):
        p = os.path.join("/opt/rocm/lib", "libamdhip64.so") if name == "amdhip64" else ctypes.util.find_library(name)
        if p and not os.path.isabs(p):
            p = next((os.path.join(d, p) for d in ("/lib/x86_64-linux-gnu", "/usr/lib/x86_64-linux-gnu", "/lib64", "/usr/lib64")
                      if os.path.exists(os.path.join(d, p))), p)
        provided |= _dynamic_symbols(p)
    assert undef - provided == set(), undef - provided
    ldd = subprocess.run(["ldd", path], capture_output=True, text=True).stdout
    assert "libsddp_hip" not in ldd


def test_user_build_is_one_unit_that_calls_nothing_of_the_core():
    """The launch sequence is the core's (csrc/sddp_api.hip): a user build brings its kernels and their launchers, defines none of
    the core's services and compiles no source but its own."""
    spec = defs.spec_of(defs.srbd13_terrain(20)[1])
    src = userterms.source(spec)
    assert "CoreHooks" not in src and "sddp_user_bind" not in src
    assert not re.search(r"\b(launch_class_\w*|launch_queue_order|alloc_cold_queue)\b", src)
    cmd = userterms._command("/tmp/unit.hip", "/tmp/unit.so")
    assert [a for a in cmd if a.endswith((".hip", ".cpp", ".cc", ".c", ".o"))] == ["/tmp/unit.hip"]
    headers = os.path.join(ROOT, "srbd_horizon_amd", "csrc")
    launch = open(os.path.join(headers, "sddp_launch.hpp")).read()
    assert "sddp_sort" not in launch and "CoreHooks" not in open(os.path.join(headers, "sddp_handle.hpp")).read()


def test_problem_without_declarations_keeps_no_user_rows():
    """A problem with no declared residual or constraint: the adapter used to return before setting its user-row state."""
    pb = SRBD13Problem()
    prb = pb.createSRBD13Problem(5, 1.0)
    prb.function_container._cost.clear()
    prb.function_container._cnstr.clear()
    s = DDPSolver.__new__(DDPSolver)
    s.prb = prb
    s.state_var, s.input_var = prb.getState().getVars(), prb.getInput().getVars()
    s.state_size = sum(v.getDim() for v in s.state_var)
    s.input_size = sum(v.getDim() for v in s.input_var)
    s._collect_constraints()
    consts = s._model_consts_from_functions()
    assert s._extra_refs == [] and s._user is None and not s._wide()
    assert "extra_rows" not in consts


def test_sym_names_and_lazy_import():
    prb = SRBD13Problem().createSRBD13Problem(5, 1.0)
    assert [s.name for s in _var(prb)["o"].sym()] == ["o_0", "o_1", "o_2", "o_3"]
    assert [s.name for s in prb.getParameters()["rdot_ref"].sym()] == ["rdot_ref_0", "rdot_ref_1", "rdot_ref_2"]
    code = "import sys; import srbd_horizon_amd, srbd_horizon_amd.ddp, srbd_horizon_amd.userterms; print('sympy' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, cwd=ROOT).stdout.strip()
    assert out == "False"
