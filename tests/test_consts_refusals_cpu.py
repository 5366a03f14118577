"""The constants no robot has are refused by name before a device is looked for (include/sddp.h): m, dt, force_scaling and lip_height
must be finite and > 0 (make_dev_consts divides by them, or a step of no length follows), a gain or weight finite and >= 0, I, com
and feet finite, lever_sign +-1, inertia_mode 0 or 1.  sddp_create and sddp_eval_knots, with and without a device: without one an
accepted neighbour of every refused value ends in "no HIP device visible", with one it makes a handle / evaluates.  (Every entry of
sddp_set_instance_consts goes through the same check; that call needs a handle: tests/test_gpu_consts.py.)"""
import ctypes as C

import numpy as np
import pytest

from oracle.cport import DIMS
from srbd_horizon_amd import _lib
from tests.consts_cases import GAINS

NO_DEVICE = "no HIP device visible: the SDDP engine has no CPU fallback"
NAN, INF = float("nan"), float("inf")
POSITIVE = ("m", "dt", "force_scaling", "lip_height")
VECTORS = {"I": 9, "com": 3, "feet": 12}
# field -> (refused values, accepted neighbours, the refusal)
CASES = {**{f: ((0.0, -1.0, NAN, INF, -INF), (1e-3, 1e-300), f + " must be finite and > 0") for f in POSITIVE},
         **{f: ((-1e-300, -1.0, NAN, INF), (0.0, 1e-300, 1e12), f + " must be finite and >= 0") for f in GAINS},
         "lever_sign": ((0.0, 0.5, 2.0, -1.5, NAN), (1.0, -1.0), "lever_sign must be +1 or -1"),
         "inertia_mode": ((-1, 2, 7), (0, 1), "inertia_mode must be 0 or 1")}
MODELS = ("srbd13", "srbd37", "lip30", "srbd61")


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _create(lib, model, c):
    h = C.c_void_p()
    rc = lib.sddp_create(C.byref(h), _lib.MODEL_IDS[model], 1, 1, None, C.byref(c))
    msg = (lib.sddp_last_error(None) or b"").decode()
    if rc == 0:
        lib.sddp_destroy(h)
    return rc, msg


def _eval(lib, model, c):
    nx, nu, npar = DIMS[model]
    nz = nx + nu
    k = np.zeros(1, dtype=np.int32)
    x, u, p = np.zeros((1, nx)), np.zeros((1, nu)), np.zeros((1, npar))
    if model != "lip30":
        x[0, 6] = 1.0      # a unit quaternion
    out = [np.zeros(n) for n in (nx, nx * nz, nz * nz, nz, 1)]
    rc = lib.sddp_eval_knots(_lib.MODEL_IDS[model], C.byref(c), 1, 1, _lib.ptr(k), _lib.ptr(x), _lib.ptr(u), _lib.ptr(p), *(_lib.ptr(a) for a in out))
    return rc, (lib.sddp_last_error(None) or b"").decode()


def _with(model, field, value, index=None):
    c = _lib.default_consts(model)
    if index is None:
        setattr(c, field, value)
    else:
        getattr(c, field)[index] = value
    return c


def _assert_refused(lib, model, c, msg):
    for call in (_create, _eval):
        rc, got = call(lib, model, c)
        assert rc == -1 and got == msg, (call.__name__, rc, got)      # SDDP_ERR_ARG, and the field by name


def _assert_accepted(lib, model, c):
    for call in (_create, _eval):
        rc, got = call(lib, model, c)
        if _has_gpu():
            assert rc == 0, (call.__name__, rc, got)
        else:
            assert rc != 0 and got == NO_DEVICE, (call.__name__, rc, got)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("field", list(CASES))
def test_a_scalar_no_robot_has_is_refused_by_name_and_its_neighbours_pass(lib, model, field):
    refused, accepted, msg = CASES[field]
    for v in refused:
        _assert_refused(lib, model, _with(model, field, v), msg)
    for v in accepted:
        _assert_accepted(lib, model, _with(model, field, v))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("field", list(VECTORS))
def test_a_non_finite_entry_of_a_vector_is_refused_by_name(lib, model, field):
    for i in (0, VECTORS[field] - 1):
        for v in (NAN, INF, -INF):
            _assert_refused(lib, model, _with(model, field, v, i), field + " holds a non-finite value")
        _assert_accepted(lib, model, _with(model, field, -1e300, i))      # finite is all that is asked of an entry


def test_the_defaults_pass_and_null_constants_are_the_defaults(lib):
    for model in _lib.MODEL_IDS:
        _assert_accepted(lib, model, _lib.default_consts(model))
    h = C.c_void_p()
    rc = lib.sddp_create(C.byref(h), 0, 1, 1, None, None)
    if rc == 0:
        lib.sddp_destroy(h)
    assert (rc == 0) if _has_gpu() else lib.sddp_last_error(None).decode() == NO_DEVICE
