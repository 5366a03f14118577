"""Cost-to-go export, what needs no GPU: the numpy recursion of tests/value_cases.py tied to the oracle's backward_pass, the two
experiments on the oracle alone (instances and eps chosen there; tests/test_gpu_value.py repeats them on the device), the bindings
against the header, and the record arithmetic."""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import ddp as oddp, models as omodels
from srbd_horizon_amd import _lib, workload
from tests import abi_header, policy_cases as pc, value_cases as vc


@pytest.mark.parametrize("model,N", [("srbd13", 30), ("srbd37", 20), ("lip30", 20)])
@pytest.mark.parametrize("gaps", ["closed", "open"])
def test_recursion_is_the_oracles_backward_pass(model, N, gaps):
    """node 0 of value_recursion against oddp.backward_pass at the warm start of a workload instance: Vx0, Vxx0, K, kff, dV1, dV2 equal
    (the same statements in the same order: exact), with closed gaps (d = 0) and with the warm start's own open gaps; Gauss-Newton
    (theta = 0), where the warm start's Quu is positive definite"""
    b = workload.make_batch(model, N, [4])
    m = omodels.make_model(model, omodels.RobotConsts(**b["consts"]))
    xs, us, P = b["xs"][0].copy(), b["us"][0], b["params"][0]
    xs[0] = b["x0"][0]
    d = oddp.defects(m, xs, us, P) if gaps == "open" else np.zeros((N, m.nx))
    if gaps == "open":
        assert np.max(np.abs(d)) > 0.0
    mu = 1e-6
    ok, K, kff, dV1, dV2, _, _, Vx0, Vxx0, _ = oddp.backward_pass(m, xs, us, P, d, mu, 0.0, 1)
    ok2, v = vc.value_recursion(m, xs, us, P, d, mu, 0.0, 1)
    assert ok and ok2
    for got, ref in ((v["vx"][0], Vx0), (v["Vxx"][0], Vxx0), (v["K"], K), (v["kff"], kff), (v["dV1"], dV1), (v["dV2"], dV2)):
        np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(v["expected"][0], -(dV1 + dV2))
    assert v["expected"][N] == 0.0 and np.all(v["Vxx"] == np.swapaxes(v["Vxx"], 1, 2))
    # c: the in-order sum of the model's costs, and the total cost but for the order of the additions
    L = [m.cost(xs[k], us[k] if k < N else None, P[k], k) for k in range(N + 1)]
    c = L[N]
    for k in range(N - 1, -1, -1):
        c = L[k] + c
        assert v["c"][k] == c
    assert abs(v["c"][0] - oddp.total_cost(m, xs, us, P)) <= 1e-12 * abs(c)
    # the terminal node is the terminal cost's own model
    _, lx, _, lxx, _, _ = m.cost_derivs(xs[N], None, P[N], N)
    np.testing.assert_array_equal(v["vx"][N], lx)
    np.testing.assert_array_equal(v["Vxx"][N], lxx)


@pytest.mark.parametrize("model", ["lip30", "srbd13"])
def test_experiments_in_the_oracle(model):
    """Check 6 on the numpy oracle alone, with the instances and eps of tests/policy_cases.py.
    Measured: lip30 |J* - word 0| / c_0 = 5.456e-16 at eps = 4e-2 and 0.0 at eps = 1e-2 (c_0 = 6667.48), recorded as
    value_cases.LIP_ORACLE_ERROR; srbd13 err 2.892e+03 / 1.823e+02 (c_0 = 97 861.5), ratio 15.86."""
    n, seed = pc.FO_CASES[model]
    b = workload.make_batch(model, n, [seed])
    m = omodels.make_model(model, omodels.RobotConsts(**b["consts"]))
    opt = oddp.DdpOptions(**pc.FO_OPTS)
    x0, P = b["x0"][0], b["params"][0]
    r = oddp.solve(m, x0, P, b["xs"][0], b["us"][0], opt)
    assert r.converged
    ref = vc.oracle_values(m, r.xs, r.us, P, dict(gap=r.gap, mu=r.mu, alpha=r.alpha, status=r.status), opt, 1)
    assert ref["ok"] == 1.0
    v = pc.fo_direction(model, m.nx)
    lin, quad, J = [], [], []
    for eps in pc.FO_EPS:
        w, _ = vc.value_at_reference(ref["c"][0], ref["expected"][0], ref["vx"][0], ref["Vxx"][0], (x0 + eps * v) - r.xs[0])
        lin.append(w[1]); quad.append(w[2])
        r2 = oddp.solve(m, x0 + eps * v, P, r.xs.copy(), r.us, opt)
        assert r2.converged
        J.append(r2.cost)
    errs = vc.value_errors(model, ref["c"][0], ref["expected"][0], lin, quad, J)
    print(f"{model}: c_0 = {ref['c'][0]:.6e}, expected_0 = {ref['expected'][0]:.3e}, lin = {lin}, quad = {quad}, J* = {J}")
    if model == "lip30":
        print(f"lip30 oracle error {max(errs):.3e} (recorded: {vc.LIP_ORACLE_ERROR:.3e})")
        assert max(errs) <= vc.LIP_ORACLE_ERROR
    vc.assert_experiment(model, errs)


def test_value_at_reference_arithmetic():
    """the reference of sddp_value_at_device: delta = 0 gives exact zeros and word 0 = c + expected; fma rounds once"""
    rng = np.random.default_rng(0)
    nx = 5
    A = rng.standard_normal((nx, nx)); A = A + A.T
    w, mag = vc.value_at_reference(3.0, 0.25, rng.standard_normal(nx), A, np.zeros(nx))
    assert w[1] == 0.0 and w[2] == 0.0 and w[0] == 3.25 and w[5] == 0.0 and mag == 3.25
    assert vc.fma(1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0) == -2.0 ** -60          # the product alone would round to 1.0
    d = rng.standard_normal(nx)
    vx = rng.standard_normal(nx)
    w, mag = vc.value_at_reference(1.0, 0.0, vx, A, d)
    assert abs(w[0] - (1.0 + vx @ d + 0.5 * d @ A @ d)) <= 4 * np.finfo(float).eps * mag and w[5] == np.max(np.abs(d))


def test_bindings_and_the_header_agree():
    """_lib declares the four calls with the header's prototypes (tests/abi_header.py), the buffer id is the header's, and the header's
    comment states the record"""
    fns = abi_header.functions()
    want = {"sddp_enable_value": ["sddp_handle* h", "int nodes"],
            "sddp_value_words": ["sddp_handle* h", "int* words", "int* nodes"],
            "sddp_fetch_value": ["sddp_handle* h", "int first", "int count", "double* out"],
            "sddp_value_at_device": ["sddp_handle* h", "int first", "int count", "int node", "const double* d_x_meas", "double* d_out"]}
    for name, params in want.items():
        assert fns[name] == ("int", params)
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == len(params)
        for decl, t in zip(params, args):
            assert abi_header.binds(decl.rsplit(" ", 1)[0], t, {}), (name, decl)
    raw = open(abi_header.HEADER).read()
    expr = re.search(r"^#define\s+SDDP_BUF_VALUE\s+\((.*?)\)", raw, flags=re.M).group(1)
    assert eval(expr, {"__builtins__": {}}, abi_header.defines()) == _lib.DEVICE_BUF_VALUE == 13
    assert abi_header.defines()["SDDP_ABI_VERSION"] == _lib.ABI_VERSION == 9
    assert "words = nodes * (nx * nx + nx + 2)" in raw and "3 784 doubles" in raw
    assert _lib.VALUE_AT_WORDS == len(_lib.VALUE_AT_FIELDS) == 8
    for nx, words in ((13, 184), (37, 1408), (30, 932), (61, 3784)):
        assert _lib.value_node_words(nx) == vc.node_words(nx) == words
    # the layout of a record, without a handle
    rec = np.arange(2 * 3 * vc.node_words(4), dtype=float).reshape(2, 3, -1)
    s = vc.split_records(rec, 4)
    assert s["c"].shape == (2, 3) and s["vx"].shape == (2, 3, 4) and s["Vxx"].shape == (2, 3, 4, 4)
    assert s["expected"][1, 2] == rec[1, 2, 1] and s["Vxx"][1, 2, 3, 1] == rec[1, 2, 2 + 4 + 3 * 4 + 1]
