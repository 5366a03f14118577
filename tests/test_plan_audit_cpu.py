"""Plan audit (include/sddp.h sddp_audit_range_device, sddp_audit), what needs no GPU: the record of tests/plan_audit_cases.py on
hand-made trajectories with known answers, the parameter names of the two declarations, and the Python signatures."""
import inspect

import numpy as np

from oracle import models as omodels
from srbd_horizon_amd import _lib
from srbd_horizon_amd.engine import DdpEngine
from srbd_horizon_amd.fleet import FleetQueue
from tests import abi_header, plan_audit_cases as pac

A = _lib
N = 5
MU = 0.8
ML = MU / np.sqrt(2.0)


def _standing(name, relative_velocity_constraints=True):
    """the model, and its static stance rolled out exactly through Model.f: x [N + 1, nx], u [N, nu], P [N + 1, np]"""
    m = omodels.make_model(name, omodels.RobotConsts(relative_velocity_constraints=relative_velocity_constraints))
    P = m.default_params(N)
    u = np.tile(m.static_input(), (N, 1))
    x = np.empty((N + 1, m.nx))
    x[0] = m.initial_state()
    for k in range(N):
        x[k + 1] = m.f(x[k], u[k], P[k])
    return m, x, u, P


def test_words_and_constants():
    assert A.AUDIT_WORDS == 16
    assert (A.AUDIT_CONE, A.AUDIT_CONE_NODE, A.AUDIT_CONE_CONTACT, A.AUDIT_PULL, A.AUDIT_PULL_NODE, A.AUDIT_SWING_LOAD, A.AUDIT_QUAT_DRIFT,
            A.AUDIT_FOOT_HEIGHT, A.AUDIT_SLIP, A.AUDIT_RIGID_FOOT, A.AUDIT_DEFECT, A.AUDIT_DEFECT_NODE, A.AUDIT_NODES,
            A.AUDIT_STANCE_PAIRS) == tuple(range(14))


def test_a_standing_plan_is_admissible_and_an_exact_rollout_has_a_rounding_level_defect():
    for name in ("srbd13", "srbd37", "srbd61"):
        m, x, u, P = _standing(name)
        rec, ops, values = pac.audit_reference(m, x, u, P, 0, MU)
        fz = m.static_input()[-1]
        assert rec[A.AUDIT_CONE] == -ML * fz < 0.0 and rec[A.AUDIT_PULL] == -fz                # no side force: -ml f_z on every contact
        assert (rec[A.AUDIT_CONE_NODE], rec[A.AUDIT_CONE_CONTACT], rec[A.AUDIT_PULL_NODE]) == (0, 0, 0)      # ties: the first
        assert rec[A.AUDIT_SWING_LOAD] == 0.0 and rec[A.AUDIT_QUAT_DRIFT] == 0.0
        assert rec[A.AUDIT_FOOT_HEIGHT] == rec[A.AUDIT_SLIP] == rec[A.AUDIT_RIGID_FOOT] == 0.0
        assert rec[A.AUDIT_DEFECT] == 0.0 and rec[A.AUDIT_DEFECT_NODE] == 0                    # x_{k+1} IS f(x_k, u_k): the same call
        assert rec[A.AUDIT_NODES] == N and rec[A.AUDIT_STANCE_PAIRS] == N * pac._parts(m)[1]["nc"] and not rec[14:].any()
        assert ops[A.AUDIT_CONE] == ML * fz
        x2 = x.copy()
        x2[3] *= 1.0 + 2.0 ** -50                                                              # a rounding-level push on one state
        r2 = pac.audit_reference(m, x2, u, P, 0, MU)[0]
        assert 0.0 < r2[A.AUDIT_DEFECT] < 1e-13 and r2[A.AUDIT_DEFECT_NODE] in (2, 3)


def test_one_foot_pushed_sideways_past_the_cone():
    m, x, u, P = _standing("srbd13")
    fz = u[3, 5]
    u = u.copy()
    u[3, 4] = -(ML * fz + 0.0625)                                           # node 3, contact 1 (the right foot), f_y
    rec, ops, values = pac.audit_reference(m, x, u, P, 0, MU)
    assert rec[A.AUDIT_CONE] == (ML * fz + 0.0625) - ML * fz and abs(rec[A.AUDIT_CONE] - 0.0625) < 1e-15
    assert (rec[A.AUDIT_CONE_NODE], rec[A.AUDIT_CONE_CONTACT]) == (3, 1)
    assert values["cone"][3, 1] == rec[A.AUDIT_CONE] and ops[A.AUDIT_CONE] == (ML * fz + 0.0625) + ML * fz
    assert rec[A.AUDIT_PULL] == -fz                                        # the side force pulls on nothing
    # a trajectory whose row 0 sits at node 2: the same place is reported as node 3
    rec2 = pac.audit_reference(m, x[2:], u[2:], P, 2, MU)[0]
    assert rec2[A.AUDIT_CONE] == rec[A.AUDIT_CONE] and (rec2[A.AUDIT_CONE_NODE], rec2[A.AUDIT_CONE_CONTACT]) == (3, 1) and rec2[A.AUDIT_NODES] == N - 2
    # the ground's coefficient: a rougher ground holds the same force
    rough = pac.audit_reference(m, x, u, P, 0, 2.0 * MU)[0]
    assert rough[A.AUDIT_CONE] == (ML * fz + 0.0625) - (2.0 * MU / np.sqrt(2.0)) * fz < 0.0
    assert np.array_equal(np.delete(rough, [A.AUDIT_CONE, A.AUDIT_CONE_NODE, A.AUDIT_CONE_CONTACT]),
                          np.delete(rec, [A.AUDIT_CONE, A.AUDIT_CONE_NODE, A.AUDIT_CONE_CONTACT]))


def test_a_pulling_foot_and_a_loaded_swing_foot():
    m, x, u, P = _standing("srbd37")
    u, P = u.copy(), P.copy()
    u[2, 6 * 2 + 5] = -0.03                                                # node 2, contact 2: f_z < 0
    P[4, m.p_sw(1)] = 0.0                                                  # node 4: contact 1 swings ...
    u[4, 6 * 1 + 3:6 * 1 + 6] = [0.01, -0.07, 0.02]                        # ... under load
    rec = pac.audit_reference(m, x, u, P, 0, MU)[0]
    assert rec[A.AUDIT_PULL] == 0.03 and rec[A.AUDIT_PULL_NODE] == 2
    assert rec[A.AUDIT_CONE] == ML * 0.03 and (rec[A.AUDIT_CONE_NODE], rec[A.AUDIT_CONE_CONTACT]) == (2, 2)
    assert rec[A.AUDIT_SWING_LOAD] == 0.07
    assert rec[A.AUDIT_STANCE_PAIRS] == 4 * N - 1


def test_quaternion_drift_and_the_contact_words():
    m, x, u, P = _standing("srbd37")
    x = x.copy()
    x[N, m.O_] *= 1.01                                                     # the last STATE node counts
    x[1, m.C_IDX[3] + 2] += 0.004                                          # contact 3 floats 4 mm at node 1
    x[2, m.CD_IDX[0]] = 0.05                                               # contact 0 slips in x at node 2 (and leaves its partner behind)
    rec = pac.audit_reference(m, x, u, P, 0, MU)[0]
    assert abs(rec[A.AUDIT_QUAT_DRIFT] - 0.01) < 1e-15
    assert abs(rec[A.AUDIT_FOOT_HEIGHT] - 0.004) < 1e-17 and rec[A.AUDIT_SLIP] == 0.05 and rec[A.AUDIT_RIGID_FOOT] == 0.05
    assert rec[A.AUDIT_DEFECT] > 1e-3                                      # none of this is a rollout any more
    m0, _, _, _ = _standing("srbd37", relative_velocity_constraints=False)
    assert pac.audit_reference(m0, x, u, P, 0, MU)[0][A.AUDIT_RIGID_FOOT] == 0.0
    assert pac.rigid_pairs(m) == [(0, 1), (2, 3)] and pac.rigid_pairs(m0) == []
    m61, _, _, _ = _standing("srbd61")
    assert pac.rigid_pairs(m61) == [(0, 1), (0, 2), (0, 3), (4, 5), (4, 6), (4, 7)]
    x[N, m.CD_IDX[1] + 1] = 9.0                                            # node N is no stage node: not read
    assert pac.audit_reference(m, x, u, P, 0, MU)[0][A.AUDIT_SLIP] == 0.05


def test_a_nan_reaches_exactly_the_words_that_read_it():
    m, x, u, P = _standing("srbd13")
    u = u.copy()
    u[1, 0] = np.nan                                                       # f_x of the left foot, in stance
    rec = pac.audit_reference(m, x, u, P, 0, MU)[0]
    nan = np.isnan(rec)
    assert sorted(np.flatnonzero(nan)) == [A.AUDIT_CONE, A.AUDIT_DEFECT]
    assert (rec[A.AUDIT_CONE_NODE], rec[A.AUDIT_CONE_CONTACT], rec[A.AUDIT_DEFECT_NODE]) == (-1, -1, -1)
    assert rec[A.AUDIT_PULL] == -u[0, 2] and rec[A.AUDIT_PULL_NODE] == 0   # f_z is there
    P = P.copy()
    P[1, m.P_SW[0]] = 0.0                                                  # the same NaN on a swing foot
    rec = pac.audit_reference(m, x, u, P, 0, MU)[0]
    assert sorted(np.flatnonzero(np.isnan(rec))) == [A.AUDIT_SWING_LOAD, A.AUDIT_DEFECT]
    assert rec[A.AUDIT_CONE_NODE] == 0 and rec[A.AUDIT_STANCE_PAIRS] == 2 * N - 1


def test_lip30_and_a_plan_without_a_stance_contact():
    m, x, u, P = _standing("lip30")
    x = x.copy()
    x[2, m.CD_IDX[2] + 1] = -0.02
    rec = pac.audit_reference(m, x, u, P, 0, MU)[0]
    assert rec[A.AUDIT_CONE] == rec[A.AUDIT_PULL] == -np.inf
    assert (rec[A.AUDIT_CONE_NODE], rec[A.AUDIT_CONE_CONTACT], rec[A.AUDIT_PULL_NODE]) == (-1, -1, -1)
    assert rec[A.AUDIT_SWING_LOAD] == rec[A.AUDIT_QUAT_DRIFT] == rec[A.AUDIT_STANCE_PAIRS] == 0.0
    assert rec[A.AUDIT_SLIP] == 0.02 and rec[A.AUDIT_RIGID_FOOT] == 0.02 and rec[A.AUDIT_NODES] == N
    m, x, u, P = _standing("srbd13")
    P = P.copy()
    P[:, list(m.P_SW)] = 0.0                                               # a flight phase over the whole horizon
    rec = pac.audit_reference(m, x, u, P, 0, MU)[0]
    assert rec[A.AUDIT_CONE] == rec[A.AUDIT_PULL] == -np.inf and rec[A.AUDIT_STANCE_PAIRS] == 0
    assert (rec[A.AUDIT_CONE_NODE], rec[A.AUDIT_CONE_CONTACT], rec[A.AUDIT_PULL_NODE]) == (-1, -1, -1)
    assert rec[A.AUDIT_SWING_LOAD] == u[0, 2]


def test_assert_record_accepts_the_reference_and_refuses_a_wrong_place():
    import pytest
    m, x, u, P = _standing("srbd13")
    u = u.copy()
    u[3, 4] = 0.5
    rec, ops, values = pac.audit_reference(m, x, u, P, 0, MU)
    assert pac.assert_record(rec, rec, ops, values, 0, 0.0) == (0.0, 0.0)
    tie = rec.copy()
    tie[A.AUDIT_PULL_NODE] = 4                                             # every node pulls alike: any of them is a maximum
    pac.assert_record(tie, rec, ops, values, 0, 0.0)
    for word, v in ((A.AUDIT_CONE_NODE, 2), (A.AUDIT_CONE, rec[A.AUDIT_CONE] * (1 + 1e-12)), (A.AUDIT_STANCE_PAIRS, 9), (A.AUDIT_DEFECT, 1e-9)):
        bad = rec.copy()
        bad[word] = v
        with pytest.raises(AssertionError):
            pac.assert_record(bad, rec, ops, values, 0, 1e-12)


def test_header_and_ctypes_agree_on_the_two_symbols():
    """the order of the integers, which no type tells apart, and what is read-only (the types: tests/test_abi.py, for every symbol)"""
    declared = abi_header.functions()
    assert declared["sddp_audit_range_device"][1] == ["sddp_handle* h", "int first", "int count", "int start", "int steps", "const double* d_x",
                                                      "const double* d_u", "double friction_coefficient", "double* d_out"]
    assert declared["sddp_audit"][1][3] == "double friction_coefficient"


def test_python_signatures():
    sig = inspect.signature(DdpEngine.audit_device)
    assert list(sig.parameters) == ["self", "out", "first", "count", "x", "u", "start", "steps", "friction"]
    assert [sig.parameters[k].default for k in ("first", "count", "x", "u", "start", "steps", "friction")] == [0, None, None, None, 0, None, 0.0]
    sig = inspect.signature(DdpEngine.audit)
    assert list(sig.parameters) == ["self", "first", "count", "friction"]
    assert [sig.parameters[k].default for k in ("first", "count", "friction")] == [0, None, 0.0]
    sig = inspect.signature(FleetQueue.flush)
    assert list(sig.parameters) == ["self", "audit_out"] and sig.parameters["audit_out"].default is None
