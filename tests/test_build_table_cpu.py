"""Which model build a (model, barrier, second_order, user rows) combination selects, or which refusal it gets: the library's
answers as literals (they were written down on the commit before the build list became a table, and passed there), and the same
set derived from srbd_horizon_amd/_lib.py INSTANCES.  Runs with and without a device: sddp_create resolves the build and validates
the constants before it looks for one, so without a GPU an existing combination ends in "no HIP device visible" and a missing one
in its own message; with a GPU an existing combination makes a handle, whose dimensions and model name are checked."""
import ctypes as C
import itertools

import pytest

from srbd_horizon_amd import _lib

MODELS = ("srbd13", "srbd37", "lip30", "srbd61")
DIMS = {"srbd13": (13, 6, 19), "srbd37": (37, 24, 19), "lip30": (30, 15, 11), "srbd61": (61, 48, 27)}
XR_COLUMNS = 8            # user rows: their per-knot references are 8 further parameter columns
COMBINATIONS = list(itertools.product(MODELS, (False, True), (False, True), (False, True)))      # (model, barrier, second_order = 2, user rows)

NO_XR = "user rows (n_extra > 0) exist for the plain builds only (no barrier, no second_order = 2)"
NO_BUILD = "this model has no such build (srbd61: no second_order = 2 build)"
NO_DEVICE = "no HIP device visible: the SDDP engine has no CPU fallback"
NO_BOUND_BARRIER = ("bound_barrier_weight > 0: the bound barrier exists for srbd13 and srbd37 only (lower / upper hold 64 entries of z; "
                    "srbd61 has 109)")
NO_EVAL_BUILD = "this model has no such build (barrier / user rows)"
# every combination that is refused, and with what; the other 21 exist (lip30's one build takes the barrier weight and second_order = 2
# without selecting anything)
REFUSED = {
    ("srbd13", True, False, True): NO_XR, ("srbd13", False, True, True): NO_XR, ("srbd13", True, True, True): NO_XR,
    ("srbd37", True, False, True): NO_XR, ("srbd37", False, True, True): NO_XR, ("srbd37", True, True, True): NO_XR,
    ("srbd61", True, False, True): NO_XR, ("srbd61", False, True, True): NO_XR, ("srbd61", True, True, True): NO_XR,
    ("srbd61", False, True, False): NO_BUILD, ("srbd61", True, True, False): NO_BUILD,
}
EXISTING = [c for c in COMBINATIONS if c not in REFUSED]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _consts(model, bar, xr, **over):
    rows = [dict(a=[1.0] + [0.0] * (DIMS[model][0] - 1), w=2.0, kind="state")] if xr else None
    return _lib.default_consts(model, friction_barrier_weight=1.0 if bar else 0.0, extra_rows=rows, **over)


def _create(lib, model, bar=False, so2=False, xr=False, **over):
    """-> (rc, handle or None, message) of sddp_create at N = 1, batch = 1"""
    h = C.c_void_p()
    opts = _lib.default_options(second_order=2 if so2 else 1)
    c = _consts(model, bar, xr, **over)
    rc = lib.sddp_create(C.byref(h), _lib.MODEL_IDS[model], 1, 1, C.byref(opts), C.byref(c))
    return rc, (h if rc == 0 else None), (lib.sddp_last_error(None) or b"").decode()


def test_the_literals_cover_all_32_combinations():
    assert len(COMBINATIONS) == 32 and len(set(COMBINATIONS)) == 32 and set(REFUSED) <= set(COMBINATIONS) and len(EXISTING) == 21


@pytest.mark.parametrize("model,bar,so2,xr", COMBINATIONS)
def test_sddp_create_selects_the_build_or_refuses_with_its_message(lib, model, bar, so2, xr):
    rc, h, msg = _create(lib, model, bar, so2, xr)
    if (model, bar, so2, xr) in REFUSED:
        assert rc != 0 and h is None and msg == REFUSED[(model, bar, so2, xr)]
        return
    if not _has_gpu():
        assert rc != 0 and h is None and msg == NO_DEVICE
        return
    assert rc == 0 and h.value, msg
    try:
        nx, nu, npar = C.c_int(), C.c_int(), C.c_int()
        assert lib.sddp_handle_dims(h, C.byref(nx), C.byref(nu), C.byref(npar)) == 0
        assert (nx.value, nu.value, npar.value) == (DIMS[model][0], DIMS[model][1], DIMS[model][2] + (XR_COLUMNS if xr else 0))
        name = C.c_char_p()
        assert lib.sddp_kernel_info(h, None, None, C.byref(name)) == 0 and name.value == model.encode()
    finally:
        lib.sddp_destroy(h)


@pytest.mark.parametrize("model", ("lip30", "srbd61"))
def test_the_bound_barrier_is_refused_where_the_bounds_do_not_fit(lib, model):
    rc, h, msg = _create(lib, model, bound_barrier_weight=1.0)
    assert rc != 0 and h is None and msg == NO_BOUND_BARRIER


@pytest.mark.parametrize("model", MODELS)
def test_sddp_eval_knots_refuses_user_rows_with_a_barrier(lib, model):
    c = _consts(model, True, True)
    rc = lib.sddp_eval_knots(_lib.MODEL_IDS[model], C.byref(c), 1, 1, *([None] * 9))
    msg = lib.sddp_last_error(None).decode()
    # lip30's one build takes the barrier weight without selecting anything: the call gets as far as its null pointers
    assert rc != 0 and msg == ("bad argument" if model == "lip30" else NO_EVAL_BUILD)


# ---- the build list itself: no library needed ---------------------------------------------------------------------------------
def _keys():
    return [(b.model, frozenset(b.traits)) for b in _lib.INSTANCES]


def test_no_two_builds_have_the_same_model_and_traits():
    keys = _keys()
    assert len(set(keys)) == len(keys) == 15
    assert len({b.fn for b in _lib.INSTANCES}) == len(keys) and len({b.type for b in _lib.INSTANCES}) == len(keys)
    for b in _lib.INSTANCES:
        assert b.model in _lib.MODEL_IDS and set(b.traits) <= {"bar", "so2", "xr"}, b


def test_the_combinations_the_library_accepts_are_the_keys_of_the_list_plus_the_lip30_rule():
    keys = set(_keys())

    def listed(model, bar, so2, xr):
        if model == "lip30":                  # its one build: barrier weight and second_order = 2 select nothing
            bar = so2 = False
        return (model, frozenset(t for t, on in (("bar", bar), ("so2", so2), ("xr", xr)) if on)) in keys
    assert [c for c in COMBINATIONS if listed(*c)] == EXISTING


def _variant_defs(defs):
    return [d for d in defs if d.startswith("-DSDDP_INST_VARIANT")]


def _inspect_defs(defs):
    return [d for d in defs if d.startswith("-DSDDP_INST_INSPECT")]


def _solve_units():
    """the units of the solve kernels: every unit but the builds' inspect units"""
    return [(name, defs) for name, defs in _lib.translation_units() if not name.endswith("_inspect")]


def test_the_resume_units_are_exactly_the_builds_without_traits():
    assert len(_lib.translation_units()) == len(set(dict(_lib.translation_units()))) == 38
    units = _solve_units()
    names = [name for name, _ in units]
    plain = sorted(b.fn for b in _lib.INSTANCES if not b.traits)
    assert _lib.VARIANTS == ("", "resume", "log")                # the order of csrc/sddp_handle.hpp SolveVariant
    assert len(set(names)) == len(names) == len(_lib.INSTANCES) + 2 * len(plain) == 23
    assert len([n for n in names if not n.endswith("_log")]) == 19
    resume = sorted(u[:-len("_resume")] for u in names if u.endswith("_resume"))
    assert resume == plain == ["lip30", "srbd13", "srbd37", "srbd61"]
    by_name = dict(units)
    for name, defs in units:
        # the one definition that says which variant a unit is: on the side units alone, the main units carry none
        side = [v for v, suffix in enumerate(_lib.VARIANTS) if v and name.endswith("_" + suffix) and name[:-len(suffix) - 1] in plain]
        assert _variant_defs(defs) == ["-DSDDP_INST_VARIANT=%d" % v for v in side], name
        assert (_variant_defs(defs) == ["-DSDDP_INST_VARIANT=1"]) == name.endswith("_resume"), name
        if name.endswith("_resume"):      # a resume unit is compiled as its build's main unit but for that definition
            assert [d for d in defs if d not in _variant_defs(defs)] == by_name[name[:-len("_resume")]], name
    assert sorted(n for n, defs in units if not _variant_defs(defs)) == sorted(b.fn for b in _lib.INSTANCES)


def test_every_build_has_exactly_one_inspect_unit_its_main_unit_plus_one_definition():
    units = _lib.translation_units()
    by_name = dict(units)
    inspect = [name for name, _ in units if name.endswith("_inspect")]
    assert sorted(inspect) == sorted(b.fn + "_inspect" for b in _lib.INSTANCES) and len(inspect) == len(set(inspect)) == 15
    assert _lib.INSPECT_DEF == "-DSDDP_INST_INSPECT"
    for name, defs in units:
        # the one definition that makes a unit the inspect unit: on the inspect units alone, once, and with no variant beside it
        assert _inspect_defs(defs) == ([_lib.INSPECT_DEF] if name in inspect else []), name
        if name in inspect:
            main = by_name[name[:-len("_inspect")]]
            assert [d for d in defs if d != _lib.INSPECT_DEF] == main and len(defs) == len(main) + 1 and not _variant_defs(defs), name
    assert _lib.compile_command("srbd61_inspect")[-3:] == ["-mllvm", "-sink-insts-to-avoid-spills", _lib.INSPECT_DEF]


def test_the_units_of_the_solve_kernels_and_their_definitions_are_what_they_were():
    """the 23 units from before the inspect units, as literals: names in build order, the definitions of one of each kind"""
    units = _solve_units()
    assert [name for name, _ in units] == [
        "srbd13", "srbd13_resume", "srbd13_log", "srbd13_b", "srbd13_s", "srbd13_bs", "srbd37", "srbd37_resume", "srbd37_log", "srbd37_b",
        "srbd37_s", "srbd37_bs", "lip30", "lip30_resume", "lip30_log", "srbd61", "srbd61_resume", "srbd61_log", "srbd13_x", "srbd37_x",
        "lip30_x", "srbd61_x", "srbd61_b"]
    by_name = dict(units)
    assert by_name["srbd13"] == ["-DSDDP_INST_MODEL=Srbd13", "-DSDDP_INST_FN=ops_srbd13", '-DSDDP_INST_NAME="srbd13"']
    assert by_name["srbd37_bs"] == ["-DSDDP_INST_MODEL=Srbd37BS", "-DSDDP_INST_FN=ops_srbd37_bs", '-DSDDP_INST_NAME="srbd37"']
    assert by_name["lip30_resume"] == ["-DSDDP_INST_MODEL=Lip30", "-DSDDP_INST_FN=ops_lip30", '-DSDDP_INST_NAME="lip30"', "-DSDDP_INST_VARIANT=1"]
    assert by_name["srbd61_log"] == ["-DSDDP_INST_MODEL=Srbd61", "-DSDDP_INST_FN=ops_srbd61", '-DSDDP_INST_NAME="srbd61"', "-mllvm",
                                     "-sink-insts-to-avoid-spills", "-DSDDP_INST_VARIANT=2"]
    for b in _lib.INSTANCES:      # every main unit: the build's three definitions and its own flags, nothing else
        assert by_name[b.fn] == ["-DSDDP_INST_MODEL=" + b.type, "-DSDDP_INST_FN=ops_" + b.fn, '-DSDDP_INST_NAME="' + b.model + '"', *b.flags]
    # the units behind them are the inspect units, so the objects of the solve kernels keep their place on the link line
    assert [name for name, _ in _lib.translation_units()][:23] == [name for name, _ in units]


def test_a_user_build_is_its_own_inspect_unit():
    """text only: the generated unit includes the inspectors' launchers and defines side_inspect_ops for its model with the macro
    csrc/sddp_inst.hip uses, in front of the make_ops that enters it"""
    import os
    import numpy as np
    from srbd_horizon_amd import userterms
    nx, nu = DIMS["srbd13"][:2]
    a = np.zeros(nx + nu)
    a[2] = 1.0
    spec = userterms.UserSpec("srbd13", nx, nu, [userterms.UserRow("state", 2.0, a=a)], [])
    src = userterms.source(spec)
    macro = "SDDP_DEFINE_INSPECT_OPS"
    assert '#include "sddp_launch_inspect.hpp"' in src and src.count(macro + "(SddpUserModel)") == 1
    assert src.index("using SddpUserModel") < src.index(macro + "(SddpUserModel)") < src.index("make_ops<sddp::SddpUserModel>")
    inst = open(os.path.join(_lib.CSRC, "sddp_inst.hip")).read()
    hdr = open(os.path.join(_lib.CSRC, "sddp_launch_inspect.hpp")).read()
    assert macro + "(SDDP_INST_MODEL)" in inst and "#define " + macro + "(M)" in hdr
    # ... and nobody writes the specialisation out by hand
    assert "side_inspect_ops<" not in src and "side_inspect_ops<SDDP" not in inst
    assert {"sddp_inspect.hpp", "sddp_launch_inspect.hpp"} <= set(_lib.HEADERS)
