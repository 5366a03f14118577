"""Time-budgeted launches (include/sddp.h sddp_set_time_budget): what can be checked without a GPU.

The feature adds two functions and nothing else to the C ABI: no struct grows, the ABI version stays 9, and the budget rides on the
resumable instantiations of the solve kernels, so the variant list and the library's translation units are what they were."""
import ctypes as C
import os
import re

from srbd_horizon_amd import _lib

HEADER = os.path.join(_lib.INCLUDE, "sddp.h")
CSRC = _lib.CSRC


def _declaration(name):
    """the argument list of `int name(...);` in the header, comments stripped"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/sddp.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_the_header_declares_the_two_functions():
    args = _declaration("sddp_set_time_budget")
    assert len(args) == 3 and "sddp_handle" in args[0] and args[1].startswith("double") and args[2].startswith("int")
    args = _declaration("sddp_time_budget_info")
    assert len(args) == 3 and "sddp_handle" in args[0] and args[1].startswith("double*") and args[2].startswith("int*")


def test_ctypes_binds_them_with_the_headers_argument_counts():
    res, args = _lib.SYMBOLS["sddp_set_time_budget"]
    assert res is C.c_int and args == [C.c_void_p, C.c_double, C.c_int]
    res, args = _lib.SYMBOLS["sddp_time_budget_info"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    for name in ("sddp_set_time_budget", "sddp_time_budget_info"):
        assert len(_lib.SYMBOLS[name][1]) == len(_declaration(name))


def test_the_abi_version_and_the_units_are_unchanged():
    src = open(HEADER).read()
    assert re.search(r"^#define SDDP_ABI_VERSION 9$", src, flags=re.M)
    assert _lib.VARIANTS == ("", "resume", "log")
    assert len(_lib.translation_units()) == 23


def test_the_argument_structs_did_not_grow():
    k = open(os.path.join(CSRC, "sddp_kernels.hpp")).read()
    assert "static_assert(sizeof(SolveArgs) == 584" in k
    assert "static_assert(sizeof(ResumeArgs) == 24" in k
    # sddp_options as the header declares it is what ctypes binds: 15 fields, none for the budget
    opts = re.search(r"typedef struct sddp_options \{(.*?)\} sddp_options;", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S), flags=re.S).group(1)
    assert len([f for f in opts.split(";") if f.strip()]) == len(_lib.SddpOptions._fields_) == 15


def test_the_device_pointer_list_names_the_clock_words():
    src = open(HEADER).read()
    assert re.search(r"\b11 time-budget clock words \[2\]", src)
