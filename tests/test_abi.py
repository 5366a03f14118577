"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and the ctypes binding is include/sddp.h,
whole: every function with its signature, every struct field by field and as the C compiler lays it out, every constant (no compute
calls without a GPU); the product path fails loudly without a device."""
import ctypes as C

import pytest

from srbd_horizon_amd import _lib
from tests import abi_header
from tests.c_host import build_c_host

STRUCTS = {"sddp_options": _lib.SddpOptions, "sddp_model_consts": _lib.SddpModelConsts, "sddp_stats": _lib.SddpStats}


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_every_function_of_the_header_is_bound_with_its_signature_and_exported(lib):
    declared = abi_header.functions()
    assert set(declared) == set(_lib.SYMBOLS), set(declared) ^ set(_lib.SYMBOLS)
    assert not set(declared) & set(_lib.DEBUG_SYMBOLS)
    for name, (ret, params) in declared.items():
        assert getattr(lib, name) is not None
        res, args = _lib.SYMBOLS[name]
        assert len(args) == len(params), (name, params, args)
        assert abi_header.binds(ret, res, STRUCTS), (name, ret, res)
        for decl, arg in zip(params, args):
            assert abi_header.binds(decl.rsplit(" ", 1)[0], arg, STRUCTS), (name, decl, arg)


def test_the_binding_rule_refuses_a_wrong_type():
    P, O, M = C.POINTER, _lib.SddpOptions, _lib.SddpModelConsts
    for ctype, good, bad in (("int", [C.c_int], [C.c_double, C.c_longlong, C.c_void_p, None]), ("double", [C.c_double], [C.c_int]),
                             ("void", [None], [C.c_int]), ("const char*", [C.c_char_p], [C.c_void_p, P(C.c_int)]),
                             ("const sddp_handle*", [C.c_void_p], [P(C.c_void_p), P(C.c_int), C.c_char_p, C.c_int]),
                             ("sddp_handle**", [C.c_void_p, P(C.c_void_p)], [P(C.c_int)]), ("void*", [C.c_void_p], [P(C.c_void_p)]),
                             ("const char**", [C.c_void_p, P(C.c_char_p)], [P(C.c_void_p), C.c_char_p]),
                             ("int*", [C.c_void_p, P(C.c_int)], [P(C.c_double), P(C.c_longlong), C.c_int, None]),
                             ("const double*", [C.c_void_p, P(C.c_double)], [P(C.c_int), C.c_double]),
                             ("long long*", [C.c_void_p, P(C.c_longlong)], [P(C.c_ulonglong), P(C.c_int)]),
                             ("const unsigned long long*", [C.c_void_p, P(C.c_ulonglong)], [P(C.c_longlong)]),
                             ("const sddp_options*", [C.c_void_p, P(O)], [P(M), P(C.c_int)]), ("float*", [C.c_void_p], [P(C.c_float)])):
        assert all(abi_header.binds(ctype, t, STRUCTS) for t in good) and not any(abi_header.binds(ctype, t, STRUCTS) for t in bad), ctype


def test_every_struct_of_the_header_is_bound_field_by_field():
    declared = abi_header.structs()
    assert set(declared) == set(STRUCTS)
    base = {C.c_int: "int", C.c_double: "double"}
    for name, S in STRUCTS.items():
        assert declared[name] == [(f, base[t._type_], t._length_) if issubclass(t, C.Array) else (f, base[t], None) for f, t in S._fields_], name
    assert [len(declared[n]) for n in ("sddp_options", "sddp_model_consts", "sddp_stats")] == [15, 30, 10]


def test_the_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    want = {name: C.sizeof(S) for name, S in STRUCTS.items()}
    want.update({name + "." + f: (getattr(S, f).offset, getattr(S, f).size) for name, S in STRUCTS.items() for f, _ in S._fields_})
    assert abi_header.compiled_layout(STRUCTS, tmp_path) == want
    dt, S = _lib.STATS_DTYPE, _lib.SddpStats
    assert dt.itemsize == C.sizeof(S) == 64                               # v9: + rho
    assert list(dt.names) == [f for f, _ in S._fields_]
    assert [(dt.fields[f][1], dt.fields[f][0].itemsize) for f in dt.names] == [(getattr(S, f).offset, getattr(S, f).size) for f in dt.names]
    # the record seen as words (engine.fetch_device_views): computed from the offsets, the values they always had
    assert (_lib.STATS_F64_WORDS, _lib.STATS_I32_WORDS, _lib.STATS_F64_COST, _lib.STATS_I32_ITERS, _lib.STATS_I32_STATUS, _lib.STATS_I32_ROLLOUTS) == (8, 16, 0, 12, 14, 15)


def test_every_constant_of_the_header_is_the_python_one(lib):
    d = abi_header.defines()
    assert _lib.ABI_VERSION == d["SDDP_ABI_VERSION"] == lib.sddp_abi_version() == 9
    assert _lib.MODEL_IDS == {k[len("SDDP_MODEL_"):].lower(): v for k, v in d.items() if k.startswith("SDDP_MODEL_")}
    assert (_lib.MAX_EXTRA, _lib.LOG_WORDS, _lib.LOG_MAX_ROWS, _lib.AUDIT_WORDS) == (8, 16, 4096, 16) \
        == (d["SDDP_MAX_EXTRA"], d["SDDP_LOG_WORDS"], d["SDDP_LOG_MAX_ROWS"], d["SDDP_AUDIT_WORDS"])
    assert len(_lib.LOG_FIELDS) == _lib.LOG_WORDS
    bufs = {k[len("SDDP_"):]: v for k, v in d.items() if k.startswith("SDDP_BUF_")}
    assert bufs == {k: v for k, v in vars(_lib).items() if k.startswith("BUF_")}
    assert list(bufs.values()) == list(range(13))                         # the ids every caller passed as bare numbers
    assert (d["SDDP_OK"], d["SDDP_ERR_ARG"], d["SDDP_ERR_HIP"], d["SDDP_ERR_MODEL"], d["SDDP_ERR_NOMEM"]) == (0, -1, -2, -3, -4)
    assert len(d) == 1 + 4 + 5 + 4 + 13                                   # and the header defines nothing this test does not know


def test_struct_layouts_and_dims(lib):
    assert _lib.model_dims("srbd13") == (13, 6, 19)
    assert _lib.model_dims("srbd37") == (37, 24, 19)
    assert _lib.model_dims("lip30") == (30, 15, 11)
    assert _lib.model_dims("srbd61") == (61, 48, 27)                      # contact_model = 4, prb.py:39-41
    assert lib.sddp_model_dims(4, None, None, None) != 0
    o = _lib.default_options()
    # Python-side defaults of the reference adapter (ddp.py:17-29)
    assert (o.max_iters, o.alpha_0, o.alpha_converge_threshold, o.line_search_decrease_factor, o.beta) == (100, 1.0, 1e-1, 0.5, 1e-4)
    c = _lib.default_consts()
    assert c.force_scaling == 1000.0 and c.dt == 0.05 and c.inertia_mode == 0 and abs(c.com[2] - 0.88) < 1e-15
    # model-aware defaults (v9): srbd61's contact points 0..3 are the first four sole corners, not the line feet
    assert list(_lib.default_consts("srbd61").feet)[:6] == [0.08, 0.13, 0.0, -0.08, 0.13, 0.0]
    assert list(_lib.default_consts("srbd37").feet) == list(c.feet) == list(_lib.default_consts("srbd13").feet)


def test_set_consts_resets_the_tail_of_the_bounds():
    """a reused constants struct keeps no stale bound beyond the values given"""
    import numpy as np
    c = _lib.default_consts(lower=[-1.0] * 19, upper=[1.0] * 19)
    assert c.lower[18] == -1.0 and c.upper[18] == 1.0
    _lib.set_consts(c, lower=[-2.0] * 13, upper=[2.0] * 13)
    assert c.lower[12] == -2.0 and c.lower[13] == -np.inf and c.upper[18] == np.inf


def test_no_cpu_fallback_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = lib.sddp_create(C.byref(h), 0, 30, 1, None, None)
    assert rc != 0 and not h.value
    assert b"no HIP device" in lib.sddp_last_error(None)
    from srbd_horizon_amd.engine import DdpEngine
    with pytest.raises(RuntimeError):
        DdpEngine("srbd13", 30, 1)


def test_c_host_program_links_against_the_abi_and_fails_loudly_without_a_device(lib, tmp_path):
    import subprocess
    import torch
    exe = build_c_host(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: tests/test_gpu_shim.py runs the program")
    r = subprocess.run([exe, "4"], capture_output=True, text=True)
    assert r.returncode != 0 and "no HIP device" in r.stderr
