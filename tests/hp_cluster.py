"""The clustering of a group of configurations (fks_cluster_configs, include/fks_capi.h) in high
precision and as a plain restatement of its definition, stated from the contract and not from the
kernels or the host twin.

matrix(): the n x n configuration distances of a group in the two backends of tests/hp_reference.py
(80-bit long double, mpmath at 40 digits), through the distance of tests/hp_policy.py.  That
distance resets its first argument; the clustering does not.  For the configurations used here the
two agree mathematically: a continuous dof or the SE(2) angle any number of turns out gives the same
wrapped difference with or without its own wrap first, and every other dof is drawn inside its
limits (asserted), so the clamp is the identity.

complete_link(): the contract's clustering on any matrix (float64, long double or mpmath objects),
with every comparison it makes optionally held against the entries' error bounds, so that a caller
learns whether a decision was near."""
import numpy as np

import hp_policy
import hp_reference as hp
from fast_kinematic_simulator_amd import _capi


def matrix(robot, configs, B=hp.DEFAULT):
    """{"d": [n][n] distances (d[i][j] from c_i to c_j), "wraps": [n][n] the sum of the wrapped terms'
    weights as hp_policy.distances counts them (c_i's own wrap to its representative, and the wrap
    of c_j minus that representative, each one term), "near_pi": [n][n] SE(3) pairs within 1e-3 of
    a half turn}"""
    W = robot.config_width
    q = np.ascontiguousarray(np.asarray(configs, dtype=np.float64).reshape(-1, W))
    if robot.robot_type == _capi.ROBOT_LINKED:
        for k, (continuous, lo, hi) in enumerate(hp_policy.dof_kinds(robot)):
            if continuous:
                assert np.all(np.abs(q[:, k]) <= 3 * np.pi), "hp_cluster.matrix: the bound's count holds for values in +-3 pi"
            else:
                assert np.all((q[:, k] >= lo) & (q[:, k] <= hi)), "hp_cluster.matrix: a limited dof outside its limits"
    elif robot.robot_type == _capi.ROBOT_SE2:
        assert np.all(np.abs(q[:, 2]) <= 3 * np.pi), "hp_cluster.matrix: the bound's count holds for angles in +-3 pi"
    out = hp_policy.distances(robot, q, q, B)
    return {"d": out["d"], "wraps": out["wraps"], "near_pi": out["near_pi"]}


def complete_link(M, threshold, bound=None):
    """The contract's clustering of one group on the matrix M (only i < j is read).  Returns
    (labels [n], count, near): near counts the decisions that two compared links, or a link and
    the threshold, leave closer than the sum of their bounds (0 without `bound` [n][n])."""
    M = np.asarray(M)
    n = M.shape[0]
    inf = float("inf")
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    S = np.full((n, n), inf, dtype=M.dtype if M.dtype != object else object)
    for i in range(n):
        for j in range(i + 1, n):
            v = M[i, j]
            S[i, j] = S[j, i] = v if v < inf else inf  # a distance that is not < +inf counts as +inf
    Bd = None
    if bound is not None:
        Bd = np.where(upper, np.asarray(bound, dtype=np.float64), 0.0)
        Bd = Bd + Bd.T
    name = np.arange(n)
    alive = np.ones(n, dtype=bool)
    near = 0
    while n > 1:
        U = np.where(upper, S, inf)
        flat = int(np.argmin(U))  # the first of the smallest in row-major order: the lowest pair
        a, b = divmod(flat, n)
        best = U[a, b]
        if not best < inf:
            break
        merging = not best > threshold
        if Bd is not None:
            if abs(float(best - threshold)) < Bd[a, b]:
                near += 1
            elif merging:
                gap = np.where(upper & (U < inf), U - best, inf)
                gap[a, b] = inf
                if np.any(gap.astype(np.float64) < Bd + Bd[a, b]):
                    near += 1
        if not merging:
            break
        row = np.where(S[b, :] > S[a, :], S[b, :], S[a, :])  # L(a u b, k) = max(L(a, k), L(b, k))
        S[a, :] = row
        S[:, a] = row
        S[a, a] = inf
        S[b, :] = inf
        S[:, b] = inf
        if Bd is not None:
            brow = np.maximum(Bd[a, :], Bd[b, :])
            Bd[a, :] = brow
            Bd[:, a] = brow
        alive[b] = False
        name[name == b] = a
    number = np.cumsum(alive) - 1  # clusters numbered in ascending order of their smallest member
    return number[name].astype(np.uint32), int(alive.sum()), near
