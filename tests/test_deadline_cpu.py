"""Time-budgeted launches (include/sddp.h sddp_set_time_budget): what can be checked without a GPU.

The feature adds two functions and nothing else to the C ABI: no struct grows, the ABI version stays 9, and the budget rides on the
resumable instantiations of the solve kernels, so the variant list and the library's translation units are what they were."""
import ctypes as C
import os

from srbd_horizon_amd import _lib
from tests import abi_header

CSRC = _lib.CSRC


def test_ctypes_binds_them_with_the_headers_argument_counts():
    res, args = _lib.SYMBOLS["sddp_set_time_budget"]
    assert res is C.c_int and args == [C.c_void_p, C.c_double, C.c_int]
    res, args = _lib.SYMBOLS["sddp_time_budget_info"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]


def test_the_abi_version_and_the_units_are_unchanged():
    assert _lib.VARIANTS == ("", "resume", "log")
    names = [name for name, _ in _lib.translation_units()]
    assert len([n for n in names if not n.endswith("_inspect")]) == 23      # the units of the solve kernels; the others: one per build
    assert len(names) == 23 + len(_lib.INSTANCES) == 38


def test_the_argument_structs_did_not_grow():
    k = open(os.path.join(CSRC, "sddp_kernels.hpp")).read()
    assert "static_assert(sizeof(SolveArgs) == 584" in k
    assert "static_assert(sizeof(ResumeArgs) == 24" in k


def test_the_device_pointer_list_names_the_clock_words():
    assert abi_header.defines()["SDDP_BUF_CLOCK"] == _lib.BUF_CLOCK == 11
