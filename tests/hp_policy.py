"""The selection of a policy table (fks_policy_table, include/fks_capi.h) in high precision,
stated from the definitions and not from the kernels or fks_policy_select:

    p   = ResetPosition(q): a joint value clamped to its limits, a continuous dof and the SE(2)
          angle taken to their representative in [-pi, pi]; an SE(3) pose as it is
    d_i = the robot's configuration distance from p to key i
          linked: sqrt(sum_k (w_k |delta_k|)^2), delta_k = key_k - p_k, wrapped for continuous dofs
          SE(2):  w0 ||delta xy|| + w1 |wrap(delta theta)|
          SE(3):  w0 ||delta t|| + w1 (the rotation angle of R^T R')

in the two backends of tests/hp_reference.py (80-bit long double, mpmath at 40 digits).  The
rotation angle is the angle whose cosine is (trace - 1) / 2 and whose sine is the norm of the
skew part's vector, taken with atan2 (well conditioned at every angle).

Everything is vectorised over configurations and keys: distances() returns [n][M] backend
arrays, and the counts the derived error bounds of tests/test_policy_cpu.py need."""
import numpy as np

import hp_reference as hp
from fast_kinematic_simulator_amd import _capi


def _map(B, fn, *arrays):
    """fn elementwise over backend arrays (numpy ufuncs for long double, python calls for mpmath)."""
    if B.kind == "longdouble":
        return fn(*arrays)
    return np.frompyfunc(fn, len(arrays), 1)(*arrays)


def _sqrt(B, x):
    return _map(B, B.sqrt, x)


def _abs(B, x):
    return np.abs(x) if B.kind == "longdouble" else np.frompyfunc(abs, 1, 1)(x)


def _atan2(B, y, x):
    return _map(B, np.arctan2 if B.kind == "longdouble" else B.mp.atan2, y, x)


def _wrap(B, x):
    """(x - 2 pi round(x / (2 pi)), whether x lay outside (-pi, pi]) elementwise"""
    two_pi = 2 * B.pi
    outside = (x <= -B.pi) | (x > B.pi)
    return x - two_pi * _map(B, B.round, x / two_pi), np.asarray(outside, dtype=bool)


def dof_kinds(robot):
    """per dof of a linked robot: (continuous, lower, upper) in dof order (the non-fixed joints)"""
    return [(j.type == _capi.JOINT_CONTINUOUS, j.lower, j.upper) for j in robot.joints if j.type != _capi.JOINT_FIXED]


def reset_position(robot, configs, B=hp.DEFAULT):
    """(p [n][W], wrapped [n][W] bool): what ResetPosition leaves of each configuration"""
    q = B.array(np.asarray(configs, dtype=np.float64).reshape(-1, robot.config_width))
    wrapped = np.zeros(q.shape, dtype=bool)
    p = q.copy()
    if robot.robot_type == _capi.ROBOT_LINKED:
        for k, (continuous, lo, hi) in enumerate(dof_kinds(robot)):
            if continuous:
                p[:, k], wrapped[:, k] = _wrap(B, q[:, k])
            else:
                lo_b, hi_b = B.scalar(lo), B.scalar(hi)
                for c in range(q.shape[0]):
                    p[c, k] = min(hi_b, max(lo_b, q[c, k]))
    elif robot.robot_type == _capi.ROBOT_SE2:
        p[:, 2], wrapped[:, 2] = _wrap(B, q[:, 2])
    return p, wrapped


def distances(robot, keys, configs, B=hp.DEFAULT):
    """{"d": [n][M] distances, "wraps": [n][M] the sum over wrapped terms of their weight (the
    reset's wrap and the difference's each count), "near_pi": [n][M] SE(3) pairs whose relative
    rotation is within 1e-3 of pi}"""
    W = robot.config_width
    p, reset_wrapped = reset_position(robot, configs, B)
    key = B.array(np.asarray(keys, dtype=np.float64).reshape(-1, W))
    n, M = p.shape[0], key.shape[0]
    w = [B.scalar(x) for x in robot.distance_weights]
    wraps = np.zeros((n, M))
    near_pi = np.zeros((n, M), dtype=bool)
    if robot.robot_type == _capi.ROBOT_LINKED:
        total = B.zeros((n, M))
        for k, (continuous, _, _) in enumerate(dof_kinds(robot)):
            delta = key[None, :, k] - p[:, None, k]
            if continuous:
                delta, outside = _wrap(B, delta)
                wraps += float(robot.distance_weights[k]) * (outside.astype(float) + reset_wrapped[:, None, k].astype(float))
            e = w[k] * _abs(B, delta)
            total = total + e * e
        d = _sqrt(B, total)
    elif robot.robot_type == _capi.ROBOT_SE2:
        dx = key[None, :, 0] - p[:, None, 0]
        dy = key[None, :, 1] - p[:, None, 1]
        dr, outside = _wrap(B, key[None, :, 2] - p[:, None, 2])
        wraps += float(robot.distance_weights[1]) * (outside.astype(float) + reset_wrapped[:, None, 2].astype(float))
        d = w[0] * _sqrt(B, dx * dx + dy * dy) + w[1] * _abs(B, dr)
    else:
        P = p.reshape(n, 3, 4)
        K = key.reshape(M, 3, 4)
        dt = K[None, :, :, 3] - P[:, None, :, 3]
        norm_t = _sqrt(B, dt[..., 0] * dt[..., 0] + dt[..., 1] * dt[..., 1] + dt[..., 2] * dt[..., 2])
        # Rel = R^T R': Rel[a][b] = sum_r R[r][a] R'[r][b]
        rel = [[sum(P[:, None, r, a] * K[None, :, r, b] for r in range(3)) for b in range(3)] for a in range(3)]
        cos_a = (rel[0][0] + rel[1][1] + rel[2][2] - 1) / 2
        vx, vy, vz = (rel[2][1] - rel[1][2]) / 2, (rel[0][2] - rel[2][0]) / 2, (rel[1][0] - rel[0][1]) / 2
        sin_a = _sqrt(B, vx * vx + vy * vy + vz * vz)
        angle = _atan2(B, sin_a, cos_a)
        near_pi = np.asarray(_abs(B, angle - B.pi) < 1e-3, dtype=bool)
        d = w[0] * norm_t + w[1] * angle
    return {"d": d, "wraps": wraps, "near_pi": near_pi}
