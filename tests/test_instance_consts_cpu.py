"""Per-instance robot constants (sddp_set_instance_consts), the part that needs no device: the `overrides` -> SddpModelConsts[count]
packing."""
import ctypes as C

import numpy as np
import pytest

from srbd_horizon_amd import _lib


def _base():
    """the defaults of sddp_default_consts_for(srbd13), without the library"""
    c = _lib.SddpModelConsts()
    _lib.set_consts(c, m=40.0, I=[2.0, 0.03, -0.02, 0.03, 1.8, 0.04, -0.02, 0.04, 0.6], com=[0, 0, 0.88], dt=0.05, force_scaling=1000.0,
                    r_tracking_gain=1e3, rdot_tracking_gain=1e4, w_tracking_gain=1e4, min_f_gain=1e-2, lip_height=0.88, lever_sign=1.0,
                    relative_velocity_constraints=1)
    return c


def test_packing_keeps_the_defaults_and_replaces_the_named_fields():
    base = _base()
    B = 5
    rng = np.random.default_rng(0)
    m = 40.0 * rng.uniform(0.75, 1.25, B)
    I = np.asarray(list(base.I)).reshape(3, 3) * rng.uniform(0.8, 1.25, B)[:, None, None]
    rows = _lib.pack_instance_consts(base, {"m": m, "I": I, "inertia_mode": np.array([0, 1, 0, 1, 1])})
    assert len(rows) == B and C.sizeof(rows) == B * C.sizeof(_lib.SddpModelConsts)
    for b in range(B):
        assert rows[b].m == m[b] and list(rows[b].I) == I[b].reshape(-1).tolist()
        assert rows[b].inertia_mode == [0, 1, 0, 1, 1][b] and isinstance(rows[b].inertia_mode, int)
        for name, _ in _lib.SddpModelConsts._fields_:                      # everything else: the base, bit for bit
            if name not in ("m", "I", "inertia_mode"):
                a, e = getattr(rows[b], name), getattr(base, name)
                assert (list(a) == list(e)) if hasattr(a, "__len__") else (a == e), name
    assert base.m == 40.0                                                  # the base itself is not touched
    flat = _lib.pack_instance_consts(base, {"I": I.reshape(B, 9), "feet": np.zeros((B, 4, 3))})
    assert list(flat[3].I) == list(rows[3].I) and list(flat[0].feet) == [0.0] * 12
    assert len(_lib.pack_instance_consts(base, {}, count=3)) == 3          # no field named: `count` copies of the base


@pytest.mark.parametrize("over,match", [
    ({"friction_barrier_weight": np.zeros(4)}, "cannot differ per instance"), ({"bound_barrier_weight": np.zeros(4)}, "cannot differ"),
    ({"lower": np.zeros((4, 64))}, "cannot differ"), ({"n_extra": np.zeros(4)}, "cannot differ"), ({"extra_rows": [()] * 4}, "cannot differ"),
    ({"friction_cone_coefficient": np.ones(4)}, "cannot differ"),
    ({"mass": np.ones(4)}, "unknown model constant"),
    ({"m": 40.0}, "one value per instance"), ({"I": np.ones((4, 3))}, "expected shape"), ({"m": np.ones((4, 2))}, "expected shape"),
    ({"m": np.ones(4), "dt": np.ones(3)}, "expected 4"), ({"m": np.array([1.0, np.nan])}, "non-finite"), ({}, "no instances")])
def test_packing_refuses_what_cannot_differ_per_instance(over, match):
    with pytest.raises(ValueError, match=match):
        _lib.pack_instance_consts(_base(), over)


def test_packing_refuses_a_base_that_is_not_a_plain_build():
    for k, v in (("friction_barrier_weight", 1e-3), ("bound_barrier_weight", 1.0), ("n_extra", 2)):
        base = _base()
        setattr(base, k, v)
        with pytest.raises(ValueError, match="plain builds"):
            _lib.pack_instance_consts(base, {"m": np.ones(2)})
