"""The summary of a group's clusters (fks_summarize_clusters, include/fks_capi.h) in high precision
and as a plain restatement, stated from the contract and not from the kernels or the host twin.

regroup(): order, count and begin of one group by the definition (a stable sort by label, the
configurations of no cluster last).

moments(): per cluster the expectation, the per-dimension variances and the scalar variance in
the two backends of tests/hp_reference.py (80-bit long double, mpmath at 40 digits), with the
numbers the derived error bounds of tests/test_summary_cpu.py need (the resultant length of every
circular mean, the norm and the eigenvalue gap of every sum of q q^T, the size of every
difference).  The rotation mean is the dominant eigenvector of sum q q^T computed in the backend
itself, by a Jacobi iteration run until the off-diagonal part is below the backend's own
precision; q follows the contract's largest-component rule, evaluated in the backend.

distance(): the robot's configuration distance between backend configurations (no reset, the
wrap inside the difference), as tests/hp_policy.py states it."""
import numpy as np

import hp_policy
import hp_reference as hp
from fast_kinematic_simulator_amd import _capi


def regroup(labels):
    """(order [n], count [n], begin [n]) of one group, positions relative to the group's start"""
    labels = [int(v) for v in labels]
    n = len(labels)
    inside = [i for i in range(n) if labels[i] < n]
    order = sorted(inside, key=lambda i: (labels[i], i)) + [i for i in range(n) if labels[i] >= n]
    count = [sum(1 for i in inside if labels[i] == c) for c in range(n)]
    begin = [sum(count[:c]) for c in range(n)]
    return order, count, begin


def circular_dims(robot):
    if robot.robot_type == _capi.ROBOT_LINKED:
        return [k for k, (continuous, _, _) in enumerate(hp_policy.dof_kinds(robot)) if continuous]
    return [2] if robot.robot_type == _capi.ROBOT_SE2 else []


def _atan2(B, y, x):
    return np.arctan2(y, x) if B.kind == "longdouble" else B.mp.atan2(y, x)


def _wrap(B, x):
    """(the representative of x in [-pi, pi], the turns taken off)"""
    turns = B.round(x / (2 * B.pi))
    return x - 2 * B.pi * turns, abs(float(turns))


def quaternion(B, T):
    """the contract's q = (w, x, y, z) of the rotation block of T (12 backend values)"""
    R = [[T[4 * i + j] for j in range(3)] for i in range(3)]
    cand = [R[0][0] + R[1][1] + R[2][2], R[0][0], R[1][1], R[2][2]]
    k = max(range(4), key=lambda a: (cand[a], -a))  # the largest, the lowest index winning a tie
    half, quarter = B.scalar(0.5), B.scalar(0.25)
    if k == 0:
        w = half * B.sqrt(1 + cand[0])
        f = quarter / w
        return [w, (R[2][1] - R[1][2]) * f, (R[0][2] - R[2][0]) * f, (R[1][0] - R[0][1]) * f]
    if k == 1:
        x = half * B.sqrt(1 + R[0][0] - R[1][1] - R[2][2])
        f = quarter / x
        return [(R[2][1] - R[1][2]) * f, x, (R[0][1] + R[1][0]) * f, (R[0][2] + R[2][0]) * f]
    if k == 2:
        y = half * B.sqrt(1 + R[1][1] - R[0][0] - R[2][2])
        f = quarter / y
        return [(R[0][2] - R[2][0]) * f, (R[0][1] + R[1][0]) * f, y, (R[1][2] + R[2][1]) * f]
    z = half * B.sqrt(1 + R[2][2] - R[0][0] - R[1][1])
    f = quarter / z
    return [(R[1][0] - R[0][1]) * f, (R[0][2] + R[2][0]) * f, (R[1][2] + R[2][1]) * f, z]


def eigen4(B, S):
    """(eigenvalues [4] descending, their unit eigenvectors as columns) of the symmetric 4 x 4
    backend matrix S: Jacobi rotations until every off-diagonal is below 1e-30 of the trace (mpmath) or
    2^-60 of it (long double, whose own rounding of the entries is 2^-64 of them)"""
    A = [[S[i][j] for j in range(4)] for i in range(4)]
    V = [[B.scalar(1.0 if i == j else 0.0) for j in range(4)] for i in range(4)]
    scale = abs(A[0][0]) + abs(A[1][1]) + abs(A[2][2]) + abs(A[3][3])
    tiny = scale * (B.scalar(1e-30) if B.kind != "longdouble" else B.scalar(2.0) ** -60)
    for _ in range(60):
        if all(abs(A[p][q]) <= tiny for p in range(3) for q in range(p + 1, 4)):
            break
        for p in range(3):
            for q in range(p + 1, 4):
                if abs(A[p][q]) <= tiny * B.scalar(1e-6):
                    continue
                theta = (A[q][q] - A[p][p]) / (2 * A[p][q])
                t = (1 if theta >= 0 else -1) / (abs(theta) + B.sqrt(theta * theta + 1))
                c = 1 / B.sqrt(t * t + 1)
                s = t * c
                for r in range(4):  # A <- A J
                    arp, arq = A[r][p], A[r][q]
                    A[r][p], A[r][q] = c * arp - s * arq, s * arp + c * arq
                for r in range(4):  # A <- J^T A
                    apr, aqr = A[p][r], A[q][r]
                    A[p][r], A[q][r] = c * apr - s * aqr, s * apr + c * aqr
                for r in range(4):
                    vrp, vrq = V[r][p], V[r][q]
                    V[r][p], V[r][q] = c * vrp - s * vrq, s * vrp + c * vrq
    else:
        raise AssertionError("hp_summary.eigen4 did not converge")
    idx = sorted(range(4), key=lambda a: -A[a][a])
    return [A[a][a] for a in idx], [[V[r][a] for a in idx] for r in range(4)]


def rotation_of(q):
    w, x, y, z = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def relative_twist(B, E, T):
    """(the body twist [v, w] of E^-1 T, its rotation angle, |t_rel|): E and T 12 backend values each, E's
    rotation block orthonormal to the backend's precision"""
    RE = [[E[4 * i + j] for j in range(3)] for i in range(3)]
    RT = [[T[4 * i + j] for j in range(3)] for i in range(3)]
    dt = [T[3] - E[3], T[7] - E[7], T[11] - E[11]]
    rel = [[sum(RE[r][a] * RT[r][b] for r in range(3)) for b in range(3)] for a in range(3)]
    t = [sum(RE[r][a] * dt[r] for r in range(3)) for a in range(3)]
    cos_a = (rel[0][0] + rel[1][1] + rel[2][2] - 1) / 2
    vee = [(rel[2][1] - rel[1][2]) / 2, (rel[0][2] - rel[2][0]) / 2, (rel[1][0] - rel[0][1]) / 2]
    s = B.sqrt(sum(v * v for v in vee))
    theta = _atan2(B, s, cos_a)
    assert float(theta) < 3.0, "hp_summary.relative_twist: a member half a turn from its cluster's mean"
    # theta / sin(theta) and the coefficient of W^2 in V^-1, by their series where theta is tiny
    if float(theta) < 1e-5:
        f = 1 + theta * theta / 6
        D = B.scalar(1.0) / 12 + theta * theta / 720
    else:
        f = theta / s
        a_coef = B.sin(theta) / theta
        b_coef = (1 - B.cos(theta)) / (theta * theta)
        D = (1 - a_coef / (2 * b_coef)) / (theta * theta)
    w = [v * f for v in vee]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    wt = cross(w, t)
    wwt = cross(w, wt)
    v = [t[k] - wt[k] / 2 + D * wwt[k] for k in range(3)]
    return v + w, theta, B.sqrt(sum(x * x for x in t))


def distance(robot, B, cfg, target):
    """(the configuration distance from cfg to target, the weight of its wrapped terms): backend values"""
    w = [B.scalar(x) for x in robot.distance_weights]
    if robot.robot_type == _capi.ROBOT_LINKED:
        total, wraps = B.scalar(0.0), 0.0
        for k, (continuous, _, _) in enumerate(hp_policy.dof_kinds(robot)):
            d = target[k] - cfg[k]
            if continuous:
                d, turns = _wrap(B, d)
                wraps += float(robot.distance_weights[k]) * turns
            e = w[k] * abs(d)
            total = total + e * e
        return B.sqrt(total), wraps
    if robot.robot_type == _capi.ROBOT_SE2:
        dx, dy = target[0] - cfg[0], target[1] - cfg[1]
        dr, turns = _wrap(B, target[2] - cfg[2])
        return w[0] * B.sqrt(dx * dx + dy * dy) + w[1] * abs(dr), float(robot.distance_weights[1]) * turns
    _, theta, _ = relative_twist(B, cfg, target)
    dt = [target[3] - cfg[3], target[7] - cfg[7], target[11] - cfg[11]]
    return w[0] * B.sqrt(sum(x * x for x in dt)) + w[1] * theta, 0.0


def moments(robot, configs, labels, B=hp.DEFAULT):
    """One group.  A list over its clusters c in [0, n): None for an empty one, otherwise a dict of
    backend values:
      "E" [W], "variances" [Wv], "variance", "members" (indices),
      "resultant" {k: the length of (sum sin, sum cos)} for every circular dimension k,
      "diff" [m][Wv] the differences the variances square, "turns" [m][Wv] the turns their wrap took off,
      "dist" [m], "dist_wraps" [m] the distances the scalar variance squares and their wrapped weight,
      "trel" [m] |t_rel| of an SE(3) member,
      "S_norm", "gap": the Frobenius norm of sum q q^T and its two largest eigenvalues' difference."""
    W = robot.config_width
    q = B.array(np.asarray(configs, dtype=np.float64).reshape(-1, W))
    n = q.shape[0]
    order, count, begin = regroup(labels)
    circ = set(circular_dims(robot))
    se3 = robot.robot_type == _capi.ROBOT_SE3
    out = []
    for c in range(n):
        m = count[c]
        if m == 0:
            out.append(None)
            continue
        mem = order[begin[c]:begin[c] + m]
        r = {"members": mem, "resultant": {}}
        if se3:
            S = [[B.scalar(0.0) for _ in range(4)] for _ in range(4)]
            for i in mem:
                qi = quaternion(B, list(q[i]))
                for a in range(4):
                    for b in range(4):
                        S[a][b] = S[a][b] + qi[a] * qi[b]
            lam, vec = eigen4(B, S)
            e = [vec[a][0] for a in range(4)]
            R = rotation_of(e)
            E = [B.scalar(0.0)] * 12
            for i3 in range(3):
                for j3 in range(3):
                    E[4 * i3 + j3] = R[i3][j3]
                E[4 * i3 + 3] = sum(q[i][4 * i3 + 3] for i in mem) / m
            r["S_norm"] = B.sqrt(sum(S[a][b] * S[a][b] for a in range(4) for b in range(4)))
            r["gap"] = lam[0] - lam[1]
            diff, trel = [], []
            for i in mem:
                tw, _, tn = relative_twist(B, E, list(q[i]))
                diff.append(tw)
                trel.append(tn)
            r["trel"] = trel
            turns = [[0.0] * 6 for _ in mem]
        else:
            E = []
            for k in range(W):
                if k in circ:
                    ss = sum(B.sin(q[i][k]) for i in mem)
                    sc = sum(B.cos(q[i][k]) for i in mem)
                    r["resultant"][k] = B.sqrt(ss * ss + sc * sc)
                    E.append(_atan2(B, ss, sc))
                else:
                    E.append(sum(q[i][k] for i in mem) / m)
            diff, turns = [], []
            for i in mem:
                row, trow = [], []
                for k in range(W):
                    d = q[i][k] - E[k]
                    t = 0.0
                    if k in circ:
                        d, t = _wrap(B, d)
                    row.append(d)
                    trow.append(t)
                diff.append(row)
                turns.append(trow)
        Wv = len(diff[0])
        r["E"] = E
        r["diff"], r["turns"] = diff, turns
        r["variances"] = [sum(row[k] * row[k] for row in diff) / m for k in range(Wv)]
        dist = [distance(robot, B, E, list(q[i])) for i in mem]
        r["dist"] = [d for d, _ in dist]
        r["dist_wraps"] = [wr for _, wr in dist]
        r["variance"] = sum(d * d for d, _ in dist) / m
        out.append(r)
    return out
