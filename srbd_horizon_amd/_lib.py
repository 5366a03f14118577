"""ctypes binding of the C ABI declared in ``include/sddp.h`` (``libsddp_hip.so``).

This is the thin Python<->HIP boundary that stands where the reference's ``import pyddp`` stands
(reference python/ddp.py:1).  There is NO CPU fallback: if the library is missing or no HIP device is visible,
the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import NamedTuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("SDDP_LIB", os.path.join(_HERE, "libsddp_hip.so"))   # SDDP_LIB: diagnostic builds only
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")

ABI_VERSION = 9      # SDDP_ABI_VERSION of include/sddp.h: what load() asks of the library
MODEL_IDS = {"srbd13": 0, "srbd37": 1, "lip30": 2, "srbd61": 3}
# the buffer ids of sddp_device_ptr (include/sddp.h SDDP_BUF_*; engine.device_buffer)
(BUF_XS, BUF_US, BUF_STATS, BUF_GAINS, BUF_X0, BUF_PARAMS, BUF_ORDER, BUF_SLOT_TIMES, BUF_POLICY, BUF_LOG, BUF_LOG_COUNTS, BUF_CLOCK,
 BUF_CLASSES) = range(13)
# ... and the value records (SDDP_BUF_VALUE, which the header derives from SDDP_BUF_CLASSES: the thirteen above are the ids that
# callers once passed as bare numbers, and tests/test_abi.py pins that set)
DEVICE_BUF_VALUE = BUF_CLASSES + 1
# ... and the two words of the last masked launch, n_selected | queue start (SDDP_BUF_SELECTED, derived in the header the same way)
DEVICE_BUF_SELECTED = BUF_CLASSES + 2


class SddpOptions(C.Structure):
    _fields_ = [("max_iters", C.c_int), ("alpha_0", C.c_double), ("alpha_converge_threshold", C.c_double),
                ("line_search_decrease_factor", C.c_double), ("beta", C.c_double), ("cost_reduction_ths", C.c_double),
                ("mu0", C.c_double), ("initial_rollout", C.c_int), ("gap_tol", C.c_double), ("mu_min", C.c_double),
                ("mu_max", C.c_double), ("second_order", C.c_int), ("waves_per_simd", C.c_int), ("queue_order", C.c_int),
                ("max_slots", C.c_int)]


class SddpModelConsts(C.Structure):
    _fields_ = [("m", C.c_double), ("I", C.c_double * 9), ("com", C.c_double * 3), ("feet", C.c_double * 12),
                ("dt", C.c_double), ("force_scaling", C.c_double),
                ("r_tracking_gain", C.c_double), ("rdot_tracking_gain", C.c_double), ("w_tracking_gain", C.c_double),
                ("rel_pos_gain", C.c_double), ("force_switch_weight", C.c_double), ("min_qddot_gain", C.c_double),
                ("min_f_gain", C.c_double), ("zmp_tracking_gain", C.c_double), ("lip_height", C.c_double),
                ("inertia_mode", C.c_int), ("lever_sign", C.c_double), ("friction_cone_coefficient", C.c_double),
                ("friction_barrier_weight", C.c_double), ("friction_barrier_sharpness", C.c_double),
                ("bound_barrier_weight", C.c_double), ("bound_barrier_sharpness", C.c_double),
                ("lower", C.c_double * 64), ("upper", C.c_double * 64), ("relative_velocity_constraints", C.c_int),
                ("n_extra", C.c_int), ("extra_kind", C.c_int * 8), ("extra_weight", C.c_double * 8), ("extra_const", C.c_double * 8),
                ("extra_a", C.c_double * 1024)]


class SddpStats(C.Structure):
    _fields_ = [("cost", C.c_double), ("alpha", C.c_double), ("gap", C.c_double), ("mu", C.c_double),
                ("expected", C.c_double), ("rho", C.c_double), ("iters", C.c_int), ("converged", C.c_int), ("status", C.c_int),
                ("rollouts", C.c_int)]


STATS_DTYPE = np.dtype([("cost", "f8"), ("alpha", "f8"), ("gap", "f8"), ("mu", "f8"), ("expected", "f8"), ("rho", "f8"),
                        ("iters", "i4"), ("converged", "i4"), ("status", "i4"), ("rollouts", "i4")])
assert STATS_DTYPE.itemsize == C.sizeof(SddpStats) == 64
LOG_WORDS, LOG_MAX_ROWS = 16, 4096      # one record of the iteration log (include/sddp.h); the largest `rows`
# the words of a record, by name
LOG_FIELDS = ("J", "A1", "B2", "rho", "gap", "expected", "alpha", "J_accepted", "theta", "mu", "tried", "slack", "iters", "rollouts",
              "mu_bumps", "reserved")
# one record of the plan audit (include/sddp.h sddp_audit_range_device), and its words by name
AUDIT_WORDS = 16
(AUDIT_CONE, AUDIT_CONE_NODE, AUDIT_CONE_CONTACT, AUDIT_PULL, AUDIT_PULL_NODE, AUDIT_SWING_LOAD, AUDIT_QUAT_DRIFT, AUDIT_FOOT_HEIGHT,
 AUDIT_SLIP, AUDIT_RIGID_FOOT, AUDIT_DEFECT, AUDIT_DEFECT_NODE, AUDIT_NODES, AUDIT_STANCE_PAIRS) = range(14)
# one record of the plan uncertainty (include/sddp.h sddp_policy_covariance_device), and its words by name
POLICY_COV_WORDS = 16
(POLICY_COV_MIN_Z, POLICY_COV_Z_NODE, POLICY_COV_Z_CONTACT, POLICY_COV_Z_ROW, POLICY_COV_MAX_TRACE, POLICY_COV_MAX_TRACE_NODE,
 POLICY_COV_TRACE, POLICY_COV_MAX_VAR, POLICY_COV_MAX_VAR_STATE, POLICY_COV_MAX_UVAR, POLICY_COV_MAX_UVAR_NODE, POLICY_COV_MAX_UVAR_INPUT,
 POLICY_COV_MIN_VAR, POLICY_COV_STEPS, POLICY_COV_OK) = range(15)
# one row of sddp_value_at_device (include/sddp.h), its words by name, and the doubles per node of a value record (sddp_value_words)
VALUE_AT_WORDS = 8
VALUE_AT_FIELDS = ("value", "lin", "quad", "c", "expected", "delta_inf", "ok", "node")


def value_node_words(nx: int) -> int:
    return nx * nx + nx + 2


# the words of one record of the stationarity certificate (include/sddp.h sddp_stationarity_range_device), by name
STATIONARITY_FIELDS = ("stationarity", "node", "input", "scale", "lambda_0", "lambda_max", "defect", "nodes")
# one record of the cost breakdown (include/sddp.h sddp_cost_terms_range_device): total | the families | largest | N.  The families'
# names are the library's (sddp_cost_terms_name): load() reads them into COST_TERM_NAMES, empty until then
COST_TERMS_WORDS, COST_TERMS_COLS = 16, 14
COST_TERM_NAMES = ()
# the words of one record of the parameter sensitivities (include/sddp.h sddp_param_gradient_range_device), by name
PARAM_GRADIENT_FIELDS = ("gradient", "node", "column", "scale", "lambda_0", "stationarity", "defect", "nodes")
# the constant sensitivities (include/sddp.h sddp_const_gradient_range_device): a record is the CONST_GRADIENT_COLS columns and the words
# CONST_GRADIENT_TAIL behind them.  The columns' names (the derived constants) and the names of the sddp_model_consts fields
# sddp_const_gradient_fields maps them to are the library's: load() reads them into CONST_GRADIENT_NAMES / CONST_GRADIENT_FIELD_NAMES
CONST_GRADIENT_WORDS, CONST_GRADIENT_COLS = 40, 32
CONST_GRADIENT_TAIL = ("relative", "column", "lambda_0", "stationarity", "defect", "nodes", "reserved0", "reserved1")
CONST_GRADIENT_NAMES = ()
CONST_GRADIENT_FIELD_NAMES = ()
# one sddp_stats record seen as words (the zero-copy device views of engine.fetch_device_views)
STATS_F64_WORDS, STATS_I32_WORDS = C.sizeof(SddpStats) // 8, C.sizeof(SddpStats) // 4
STATS_F64_COST = SddpStats.cost.offset // 8
STATS_I32_ITERS, STATS_I32_STATUS, STATS_I32_ROLLOUTS = (getattr(SddpStats, f).offset // 4 for f in ("iters", "status", "rollouts"))

_P = C.POINTER
_dp = _P(C.c_double)
_vp = C.c_void_p

# every symbol include/sddp.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sddp_abi_version": (C.c_int, []),
    "sddp_model_dims": (C.c_int, [C.c_int, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "sddp_handle_dims": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "sddp_default_options": (None, [_P(SddpOptions)]),
    "sddp_default_consts": (None, [_P(SddpModelConsts)]),
    "sddp_default_consts_for": (C.c_int, [C.c_int, _P(SddpModelConsts)]),
    "sddp_set_params": (C.c_int, [_vp, _vp]),
    "sddp_advance": (C.c_int, [_vp, _vp, _vp]),
    "sddp_solve_resident": (C.c_int, [_vp, _vp, _vp, _vp]),
    "sddp_solve_resident_first": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "sddp_model_step": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp]),
    "sddp_create": (C.c_int, [_P(_vp), C.c_int, C.c_int, C.c_int, _P(SddpOptions), _P(SddpModelConsts)]),
    "sddp_destroy": (None, [_vp]),
    "sddp_last_error": (C.c_char_p, [_vp]),
    "sddp_set_options": (C.c_int, [_vp, _P(SddpOptions)]),
    "sddp_set_initial_state": (C.c_int, [_vp, _vp]),
    "sddp_set_x_warmstart": (C.c_int, [_vp, _vp]),
    "sddp_set_u_warmstart": (C.c_int, [_vp, _vp]),
    "sddp_solve": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "sddp_is_converged": (C.c_int, [_vp, _vp]),
    "sddp_set_stream": (C.c_int, [_vp, _vp]),
    "sddp_set_initial_state_device": (C.c_int, [_vp, _vp]),
    "sddp_set_x_warmstart_device": (C.c_int, [_vp, _vp]),
    "sddp_set_u_warmstart_device": (C.c_int, [_vp, _vp]),
    "sddp_solve_device": (C.c_int, [_vp, _vp]),
    "sddp_load_range_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "sddp_solve_range_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "sddp_record_words": (C.c_int, [_vp, C.c_int, _P(C.c_int)]),
    "sddp_pack_records_device": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    "sddp_enable_policy": (C.c_int, [_vp, C.c_int]),
    "sddp_policy_words": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "sddp_policy_range_device": (C.c_int, [_vp, C.c_int, C.c_int]),
    "sddp_fetch_policy": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "sddp_apply_policy_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "sddp_apply_policy_knot_device": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "sddp_policy_rollout_device": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "sddp_enable_value": (C.c_int, [_vp, C.c_int]),
    "sddp_value_words": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "sddp_fetch_value": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "sddp_value_at_device": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "sddp_policy_covariance_words": (C.c_int, [_vp, _P(C.c_int)]),
    "sddp_policy_covariance_device": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp]),
    "sddp_audit_range_device": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_double, _vp]),
    "sddp_audit": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _vp]),
    "sddp_stationarity_words": (C.c_int, [_vp, _P(C.c_int)]),
    "sddp_stationarity_range_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "sddp_stationarity": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "sddp_cost_terms_words": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "sddp_cost_terms_name": (C.c_int, [C.c_int, _P(C.c_char_p)]),
    "sddp_cost_terms_range_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "sddp_cost_terms": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "sddp_param_gradient_words": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "sddp_param_gradient_range_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "sddp_param_gradient": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "sddp_const_gradient_words": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "sddp_const_gradient_name": (C.c_int, [C.c_int, _P(C.c_char_p)]),
    "sddp_const_gradient_range_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "sddp_const_gradient": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "sddp_const_gradient_fields": (C.c_int, [_P(SddpModelConsts), _vp, _vp, _P(C.c_int)]),
    "sddp_const_gradient_field_name": (C.c_int, [C.c_int, _P(C.c_char_p)]),
    "sddp_enable_resume": (C.c_int, [_vp, C.c_int]),
    "sddp_continue_range_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "sddp_continue_device": (C.c_int, [_vp, _vp]),
    "sddp_continue_resident": (C.c_int, [_vp]),
    "sddp_unfinished_count": (C.c_int, [_vp, C.c_int, C.c_int, _P(C.c_int)]),
    "sddp_set_time_budget": (C.c_int, [_vp, C.c_double, C.c_int]),
    "sddp_time_budget_info": (C.c_int, [_vp, _P(C.c_double), _P(C.c_int)]),
    "sddp_solve_masked_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp]),
    "sddp_continue_masked_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp]),
    "sddp_policy_masked_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "sddp_advance_masked_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "sddp_last_selected": (C.c_int, [_vp, _P(C.c_int)]),
    "sddp_enable_iteration_log": (C.c_int, [_vp, C.c_int]),
    "sddp_iteration_log_info": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "sddp_fetch_iteration_log": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "sddp_set_instance_classes": (C.c_int, [_vp, _vp, C.c_int]),
    "sddp_set_instance_classes_range_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int]),
    "sddp_class_history": (C.c_int, [_vp, C.c_int, _P(C.c_double), _P(C.c_longlong)]),
    "sddp_enable_auto_classes": (C.c_int, [_vp, C.c_int]),
    "sddp_auto_classes_info": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "sddp_fetch_instance_classes": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "sddp_get_class_stats": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "sddp_add_class_stats": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "sddp_set_instance_consts": (C.c_int, [_vp, C.c_int, C.c_int, _P(SddpModelConsts)]),
    "sddp_clear_instance_consts": (C.c_int, [_vp]),
    "sddp_instance_consts_active": (C.c_int, [_vp, _P(C.c_int)]),
    "sddp_queue_info": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "sddp_fetch": (C.c_int, [_vp, _vp, _vp, _vp]),
    "sddp_synchronize": (C.c_int, [_vp]),
    "sddp_kernel_info": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int), _P(C.c_char_p)]),
    "sddp_kernel_resources": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "sddp_debug_poison_lds": (C.c_int, [_vp]),
    "sddp_device_ptr": (C.c_int, [_vp, C.c_int, _P(_vp), _P(C.c_longlong)]),
    "sddp_last_kernel_ms": (C.c_int, [_vp, _P(C.c_double)]),
    "sddp_enable_timing": (C.c_int, [_vp, C.c_int]),
    "sddp_kernel_time_stats": (C.c_int, [_vp, _P(C.c_double), _P(C.c_longlong), C.c_int]),
    "sddp_eval_knots": (C.c_int, [C.c_int, _P(SddpModelConsts), C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sddp_register_user_build": (C.c_int, [C.c_char_p, _P(C.c_int)]),
    "sddp_backward": (C.c_int, [_vp, _vp, C.c_double, _vp, _vp]),
    "sddp_forward": (C.c_int, [_vp, _vp, C.c_double, _vp, _vp, _vp]),
}
# diagnostics the library exports beside include/sddp.h (not part of the ABI)
DEBUG_SYMBOLS = {
    "sddp_debug_set_phase_mode": (C.c_int, [_vp, C.c_double, C.c_int]),      # theta, closed: how sddp_backward / sddp_forward run
}

_lib = None


class Build(NamedTuple):
    """One model build of the library: the units of csrc/sddp_inst.hip (translation_units) behind the accessor sddp::ops_<fn>()."""
    fn: str                 # accessor suffix
    type: str               # device model type (csrc/sddp_models.hpp)
    model: str              # model name, a key of MODEL_IDS
    traits: tuple = ()      # of "bar" (barrier build), "so2" (full second order), "xr" (user rows): the type's BAR, SO2, NXR > 0
    flags: tuple = ()       # compiler options of this build alone


# srbd61 (one workgroup per CU, 512 registers a lane, still 1.8 KB of scratch): LLVM's -sink-insts-to-avoid-spills moves hoisted
# loop-invariant address arithmetic back into the loops instead of spilling it: 25.8 -> 27.3 k solves/s when it went in, 31.8 -> 32.3 k
# on the round's final kernel (profiles/r04/experiments/README.md).  Measured and NOT applied elsewhere: srbd13 -1 % (scratch
# 524 -> 288 B but slower), srbd37 +2.3 % in the two-per-SIMD build and -3 % in the other, which share a translation unit.
_SINK = ("-mllvm", "-sink-insts-to-avoid-spills")
# THE list of model builds: what build() compiles and hands to csrc/sddp_api.hip, which finds a handle's build in it by
# (model, traits); no two entries share that key (build() checks).  The builds without traits are the plain builds: they alone have
# table kernels (sddp_set_instance_consts) and the solve kernels' further variants (VARIANTS: sddp_enable_resume,
# sddp_enable_iteration_log), each compiled in a translation unit of its own; every build has one more unit for the kernels that only
# read a plan (translation_units).  A new build: its alias in csrc/sddp_models.hpp and one entry here.
INSTANCES = [
    Build("srbd13", "Srbd13", "srbd13"), Build("srbd13_b", "Srbd13B", "srbd13", ("bar",)),
    Build("srbd13_s", "Srbd13S", "srbd13", ("so2",)), Build("srbd13_bs", "Srbd13BS", "srbd13", ("bar", "so2")),
    Build("srbd37", "Srbd37", "srbd37"), Build("srbd37_b", "Srbd37B", "srbd37", ("bar",)),
    Build("srbd37_s", "Srbd37S", "srbd37", ("so2",)), Build("srbd37_bs", "Srbd37BS", "srbd37", ("bar", "so2")),
    Build("lip30", "Lip30", "lip30"), Build("srbd61", "Srbd61", "srbd61", (), _SINK),
    Build("srbd13_x", "Srbd13X", "srbd13", ("xr",)), Build("srbd37_x", "Srbd37X", "srbd37", ("xr",)), Build("lip30_x", "Lip30X", "lip30", ("xr",)),
    Build("srbd61_x", "Srbd61X", "srbd61", ("xr",), _SINK), Build("srbd61_b", "Srbd61B", "srbd61", ("bar",), _SINK),
]
HEADERS = ["sddp_kernels.hpp", "sddp_kernels_mw.hpp", "sddp_models.hpp", "sddp_sort.hpp", "sddp_handle.hpp", "sddp_launch.hpp", "sddp_kernels_host.hpp",
           "sddp_inspect.hpp", "sddp_launch_inspect.hpp"]


def header_stamp(root: str = ROOT) -> str:
    """Stamp of the headers a model build is compiled against (csrc/*.hpp of HEADERS, include/sddp.h): the core library and every
    user build carry it (-DSDDP_HEADER_STAMP), and sddp_register_user_build refuses a build whose stamp differs."""
    import hashlib
    h = hashlib.sha1()
    for p in [os.path.join(root, "srbd_horizon_amd", "csrc", n) for n in HEADERS] + [os.path.join(root, "include", "sddp.h")]:
        h.update(open(p, "rb").read())
    return "0x" + h.hexdigest()[:15]


# the solve variants, in the order of csrc/sddp_handle.hpp SolveVariant: the suffix of a variant's translation units
VARIANTS = ("", "resume", "log")
# the one definition that makes csrc/sddp_inst.hip a build's inspect unit
INSPECT_DEF = "-DSDDP_INST_INSPECT"


def build_jobs() -> int:
    """How many compilers run at once: the first of SDDP_BUILD_JOBS, MAX_JOBS, CMAKE_BUILD_PARALLEL_LEVEL that is set, else the CPUs
    the host reports, at most 16 (a shared machine reports hundreds and allows far fewer)."""
    for var in ("SDDP_BUILD_JOBS", "MAX_JOBS", "CMAKE_BUILD_PARALLEL_LEVEL"):
        if os.environ.get(var):
            return max(1, int(os.environ[var]))
    return min(os.cpu_count() or 4, 16)


def translation_units():
    """Every translation unit of csrc/sddp_inst.hip that build() compiles and links, as (unit name, definitions and options): the main
    unit of every entry of INSTANCES, named by its accessor suffix, and for every build without traits one side unit
    <suffix>_<variant> per further entry of VARIANTS: that variant's solve kernels and their launcher (-DSDDP_INST_VARIANT=<index>),
    which the main unit enters in its table.  A side unit is its main unit's command line plus that one definition; a build with
    traits that asked for one would not compile (csrc/sddp_launch.hpp launch_solve_variant).  Behind them, for every entry of
    INSTANCES, its inspect unit <suffix>_inspect (INSPECT_DEF): the kernels that only read a plan (csrc/sddp_inspect.hpp), kept out
    of the device modules of the solve kernels; again its main unit's command line plus the one definition."""
    def main(b):
        return ["-DSDDP_INST_MODEL=" + b.type, "-DSDDP_INST_FN=ops_" + b.fn, '-DSDDP_INST_NAME="' + b.model + '"', *b.flags]
    return ([(b.fn + ("_" + suffix if v else ""), main(b) + (["-DSDDP_INST_VARIANT=%d" % v] if v else []))
             for b in INSTANCES for v, suffix in enumerate(VARIANTS) if v == 0 or not b.traits]
            + [(b.fn + "_inspect", main(b) + [INSPECT_DEF]) for b in INSTANCES])


def compile_command(unit: str | None = None, root: str = ROOT) -> list:
    """The head of every compile command of the library's HIP sources: the compiler, its flags, the include paths of the tree at
    `root` and, for a unit of translation_units(), that unit's definitions.  The tail is the caller's: -c or -shared, source, output."""
    head = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC",
            "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "srbd_horizon_amd", "csrc")]
    return head + (dict(translation_units())[unit] if unit is not None else [])


def _newer(target: str, deps) -> bool:
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)


def _cmd_stamp(obj: str) -> str:
    return obj + ".cmd"


def _fresh(obj: str, deps, cmd) -> bool:
    """An object is fresh when it is newer than its sources AND was compiled by exactly this command line (flags, defines)."""
    if not _newer(obj, deps):
        return False
    try:
        return open(_cmd_stamp(obj)).read() == " ".join(cmd)
    except OSError:
        return False


def build(force: bool = False, verbose: bool = False, only=None) -> str:
    """Compile the HIP library for gfx950 into libsddp_hip.so (in-tree, so it travels to the GPU box): the host API
    (csrc/sddp_api.hip), the queue sort (csrc/sddp_sort.hip) and one object per unit of the model builds (csrc/sddp_inst.hip x
    translation_units()), compiled in parallel (build_jobs) and linked.  Objects live in build/obj (git-ignored), each beside a stamp of the command line that
    made it; stale ones (older than a source or header, or made by another command line) are recompiled.
    only: recompile just these model builds (development); refuses to link while another object is stale."""
    import hashlib
    from concurrent.futures import ThreadPoolExecutor
    keys = [(b.model, frozenset(b.traits)) for b in INSTANCES]
    if len(set(keys)) != len(keys) or any(b.model not in MODEL_IDS for b in INSTANCES):
        raise RuntimeError("INSTANCES: two builds of one model with the same traits, or a model name that MODEL_IDS does not know")
    extra = os.environ.get("SDDP_CXXFLAGS", "").split()      # diagnostic builds only (-DSDDP_STAMPS), with SDDP_LIB
    default = LIB_PATH.endswith("libsddp_hip.so") and not extra
    tag = "" if default else "_" + hashlib.sha1(repr((LIB_PATH, tuple(extra))).encode()).hexdigest()[:10]
    objdir = os.path.join(ROOT, "build", "obj" + tag)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(INCLUDE, "sddp.h")]
    srcs = [os.path.join(CSRC, n + ".hip") for n in ("sddp_api", "sddp_sort", "sddp_inst")]
    if not force and only is None and not os.path.isdir(objdir) and _newer(LIB_PATH, srcs + hdrs):
        return LIB_PATH                                      # a shipped library newer than every source: nothing to do
    os.makedirs(objdir, exist_ok=True)
    # sddp_api.hip names no build: it gets the accessors of INSTANCES as an X-macro list, and the stamp of the headers (user builds:
    # userterms.py)
    api_defs = [f"-DSDDP_HEADER_STAMP={header_stamp()}ULL", "-DSDDP_BUILDS=" + " ".join(f"X(ops_{b.fn})" for b in INSTANCES)]
    jobs = []
    for name, defs in (("sddp_api", api_defs), ("sddp_sort", [])):
        src = os.path.join(CSRC, name + ".hip")
        obj = os.path.join(objdir, name + ".o")
        jobs.append((obj, src, compile_command() + extra + defs + ["-c", src, "-o", obj]))
    inst = os.path.join(CSRC, "sddp_inst.hip")
    for unit, _ in translation_units():
        obj = os.path.join(objdir, "inst_" + unit + ".o")
        jobs.append((obj, inst, compile_command(unit) + extra + ["-c", inst, "-o", obj]))
    todo, left_stale = [], []
    for obj, src, cmd in jobs:
        picked = only is not None and any(obj.endswith("inst_" + o + ".o") for o in only)
        if force or picked or not _fresh(obj, [src] + hdrs, cmd):
            if only is not None and not picked and not force:
                left_stale.append(os.path.basename(obj))
                continue
            todo.append((obj, src, cmd))
    if left_stale:
        raise RuntimeError(f"build(only={only}): {left_stale} are stale too; build without `only` first")
    if not todo and _newer(LIB_PATH, [j[0] for j in jobs]):
        return LIB_PATH

    def compile_one(job):
        obj, src, cmd = job
        if verbose:
            print(" ".join(cmd), flush=True)
        if os.path.exists(_cmd_stamp(obj)):
            os.remove(_cmd_stamp(obj))
        subprocess.run(cmd, check=True)
        with open(_cmd_stamp(obj), "w") as f:
            f.write(" ".join(cmd))

    workers = max(1, min(len(todo), build_jobs()))
    if todo:
        with ThreadPoolExecutor(max_workers=workers) as ex:
            list(ex.map(compile_one, todo))
    link = [compile_command()[0], "--offload-arch=gfx950", "-shared", "-fPIC", *[j[0] for j in jobs], "-o", LIB_PATH]
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.run(link, check=True)
    return LIB_PATH


def load():
    """dlopen the HIP library and type every symbol of include/sddp.h.  Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the DDP engine)")
    try:
        # PyTorch bundles its own HIP runtime with the same soname (libamdhip64.so.7).  Load it first so the process has
        # ONE HIP runtime shared by torch tensors / streams and this library (loading the system one first and torch's
        # second leaves this library without a visible device).
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SYMBOLS, **DEBUG_SYMBOLS}.items():
        fn = getattr(lib, name)      # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.sddp_abi_version() != ABI_VERSION:
        raise RuntimeError("libsddp_hip.so ABI version mismatch")
    global COST_TERM_NAMES
    names, name = [], C.c_char_p()
    while lib.sddp_cost_terms_name(len(names), C.byref(name)) == 0:
        names.append(name.value.decode())
    COST_TERM_NAMES = tuple(names)
    global CONST_GRADIENT_NAMES, CONST_GRADIENT_FIELD_NAMES
    for fn, target in ((lib.sddp_const_gradient_name, "CONST_GRADIENT_NAMES"), (lib.sddp_const_gradient_field_name, "CONST_GRADIENT_FIELD_NAMES")):
        names = []
        while fn(len(names), C.byref(name)) == 0:
            names.append(name.value.decode())
        globals()[target] = tuple(names)
    _lib = lib
    return lib


def default_options(**over) -> SddpOptions:
    o = SddpOptions()
    load().sddp_default_options(C.byref(o))
    for k, v in over.items():
        if not hasattr(o, k):
            raise KeyError(f"unknown option {k!r}")
        setattr(o, k, v)
    return o


def default_consts(model: str | None = None, **over) -> SddpModelConsts:
    """The synthetic robot as `model` needs it (sddp_default_consts_for: srbd61's `feet` are the first four sole corners of the
    eight-point contact model); model None = the line-foot robot of sddp_default_consts."""
    c = SddpModelConsts()
    if model is None:
        load().sddp_default_consts(C.byref(c))
    else:
        check(load().sddp_default_consts_for(MODEL_IDS[model], C.byref(c)))
    set_consts(c, **over)
    return c


MAX_EXTRA = 8


def _set_extra_rows(c: SddpModelConsts, rows):
    """rows: sequence of dict(a [nx + nu], w, kind "state" | "stage", const) -- user-declared linear residual rows
    sqrt(w) (a . z - (p[np + j] + const)) (include/sddp.h extra_*); None / () clears them."""
    rows = list(rows or ())
    if len(rows) > MAX_EXTRA:
        raise ValueError(f"at most {MAX_EXTRA} extra rows")
    c.n_extra = len(rows)
    for j in range(MAX_EXTRA):
        c.extra_kind[j] = 0
        c.extra_weight[j] = c.extra_const[j] = 0.0
        for i in range(128):
            c.extra_a[128 * j + i] = 0.0
    for j, r in enumerate(rows):
        a = np.asarray(r["a"], dtype=float).reshape(-1)
        if a.size > 128:
            raise ValueError("extra row: at most 128 coefficients")
        if r["kind"] not in ("state", "stage"):
            raise ValueError("extra row kind must be 'state' or 'stage'")
        c.extra_kind[j] = 0 if r["kind"] == "state" else 1
        c.extra_weight[j] = float(r["w"])
        c.extra_const[j] = float(r.get("const", 0.0))
        for i, v in enumerate(a):
            c.extra_a[128 * j + i] = float(v)


def set_consts(c: SddpModelConsts, **over):
    for k, v in over.items():
        if k == "extra_rows":
            _set_extra_rows(c, v)
            continue
        if k in ("lower", "upper"):                    # bounds of z = [x u]: the first nx + nu entries, the rest stays unbounded
            field = getattr(c, k)
            if v is not None:
                arr = np.asarray(v, dtype=float).reshape(-1)
                if arr.size > len(field):
                    raise ValueError(f"{k}: at most {len(field)} values")
                for i in range(len(field)):              # the tail is reset: a reused struct keeps no stale bound
                    field[i] = float(arr[i]) if i < arr.size else (-np.inf if k == "lower" else np.inf)
        elif k in ("I", "com", "feet"):
            arr = np.asarray(v, dtype=float).reshape(-1)
            field = getattr(c, k)
            if arr.size != len(field):
                raise ValueError(f"{k}: expected {len(field)} values")
            for i, a in enumerate(arr):
                field[i] = float(a)
        elif hasattr(c, k):
            setattr(c, k, v)
        else:
            raise KeyError(f"unknown model constant {k!r}")
    return c


# what sddp_set_instance_consts lets differ from one instance to the next (include/sddp.h): field -> trailing shape of its override
INSTANCE_CONST_FIELDS = {"m": (), "I": (9,), "com": (3,), "feet": (12,), "dt": (), "force_scaling": (), "r_tracking_gain": (),
                         "rdot_tracking_gain": (), "w_tracking_gain": (), "rel_pos_gain": (), "force_switch_weight": (),
                         "min_qddot_gain": (), "min_f_gain": (), "zmp_tracking_gain": (), "lip_height": (), "inertia_mode": (),
                         "lever_sign": (), "relative_velocity_constraints": ()}
_INT_CONST_FIELDS = ("inertia_mode", "relative_velocity_constraints")


def pack_instance_consts(base: SddpModelConsts, overrides: dict, count: int | None = None):
    """overrides: field -> array [count, ...] (I as [count, 3, 3] or [count, 9], feet as [count, 4, 3] or [count, 12], scalars as
    [count]) -> a ctypes array SddpModelConsts[count], every entry a copy of `base` with the named fields replaced.  Fields that
    select a kernel build or a device side table (barrier weights, bounds, user rows) cannot differ per instance: ValueError, like
    an unknown field or a shape that does not fit.  Needs no device."""
    if base.n_extra != 0 or base.friction_barrier_weight != 0.0 or base.bound_barrier_weight != 0.0:
        raise ValueError("per-instance constants exist for plain builds only (no user rows, no barrier)")
    cols = {}
    for k, v in overrides.items():
        if k not in INSTANCE_CONST_FIELDS:
            known = hasattr(base, k) or k == "extra_rows"
            raise ValueError(f"{k!r} cannot differ per instance (it selects a kernel build or a device side table)" if known
                             else f"unknown model constant {k!r}")
        a = np.asarray(v, dtype=np.float64)
        if a.ndim < 1:
            raise ValueError(f"{k}: expected one value per instance, shape [count, ...]")
        n = a.shape[0]
        width = int(np.prod(INSTANCE_CONST_FIELDS[k], dtype=int))
        if a.size != n * width:
            raise ValueError(f"{k}: expected shape [count{''.join(', %d' % d for d in INSTANCE_CONST_FIELDS[k])}], got {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{k}: non-finite value")
        if count is None:
            count = n
        if n != count:
            raise ValueError(f"{k}: {n} instances, expected {count}")
        cols[k] = a.reshape(n, width)
    if count is None or count < 1:
        raise ValueError("no instances: give at least one override or a count >= 1")
    out = (SddpModelConsts * count)()
    for i in range(count):
        C.memmove(C.byref(out[i]), C.byref(base), C.sizeof(SddpModelConsts))
        for k, a in cols.items():
            if INSTANCE_CONST_FIELDS[k]:
                field = getattr(out[i], k)
                for j in range(a.shape[1]):
                    field[j] = a[i, j]
            else:
                setattr(out[i], k, int(a[i, 0]) if k in _INT_CONST_FIELDS else float(a[i, 0]))
    return out


def check(rc: int, handle=None):
    if rc != 0:
        msg = load().sddp_last_error(handle)
        raise RuntimeError(f"sddp error {rc}: {msg.decode() if msg else '?'}")


def ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def model_dims(model: str):
    nx, nu, npar = C.c_int(), C.c_int(), C.c_int()
    check(load().sddp_model_dims(MODEL_IDS[model], C.byref(nx), C.byref(nu), C.byref(npar)))
    return nx.value, nu.value, npar.value
