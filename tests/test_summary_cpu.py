"""fks_summarize_clusters, the host twin of the summary kernels, without a GPU: its regrouping,
counts and reached against a plain restatement (exactly), its expectations and variances against
the high-precision statement of tests/hp_summary.py within bounds counted below, hand cases on a
robot whose arithmetic is exact, and a continuous dof whose members straddle +-pi.

The bounds, operation by operation (u = 2^-53, m the cluster's members, every bound times
1 + 2^-40 for the second-order terms; the inputs are float64 values taken exactly):

  linear mean   a serial sum of m terms errs by at most (m - 1) u sum|x_i|, the division by u |E|:
                at most m u X, X = max |x_i|.
  circular mean sin and cos of the portable libm are below 1 ulp, so a term errs by at most 2 u; the
                serial sums (sum |s_i| <= m) by (m - 1) u m: each of (S, C) by e = m u (m + 1).  The
                angle of (S, C) then moves by at most sqrt(2) e / (r - sqrt(2) e), r the resultant
                length: the term carries 1 / r.  atan2 is below 1 ulp: 2 u pi more.  The comparison
                is of angles (modulo a turn).
  rotation mean a quaternion component by Shepperd's rule: the selected 4 c^2 is at least 1 and at
                most 4, three additions of values up to 4 (9 u), the root (4.5 u + 2 u), halved:
                3.25 u; f = 0.25 / c to 7.5 u relative; a component (difference, f, product, all at
                most 1) 9.5 u: 10 u each.  A product q_a q_b: 21 u; an entry of S (sum |q_a q_b| <=
                m): m u (21 + m - 1); its 16 entries: |dS|_F <= 4 m u (m + 20).  The dominant
                eigenvector of S + dS leaves that of S by at most 2 |dS|_F / gap (Davis-Kahan),
                gap the difference of S's two largest eigenvalues.  The Jacobi iteration: at most
                16 sweeps of 6 rotations; a rotation computes t to 6 u, c to 9 u and s to 16 u
                relative, so the entry it declares zero is off by 16 u |A|, the rotation is
                orthogonal to 18 u, and each updated entry (two products, a difference) adds 5 u:
                40 u |A|_F backward error per rotation, 96 x 40 = 3840 u |S|_F in all, felt in the
                eigenvector as 3840 u |S|_F / gap: the term carries the matrix norm over the gap.
                V gathers 18 u + 5 u per rotation, 2208 u; the normalisation 4 u.  So the unit
                quaternion errs by dq = (2 |dS|_F + 3840 u |S|_F) / gap + 2212 u, an entry of the
                rotation block (quadratic, |w| + |x| + |y| + |z| <= 2) by 4 dq + 4 u, and the
                rotation itself by the angle dphi = 2 dq + 8 u.
  variances     a difference d_i = c_i - E inherits E's error dE and its own rounding u |raw|; a
                wrapped one also 2.21 u per turn taken off (the float64 2 pi; the remainder and
                its final step are exact): eta = dE + u |raw| + 2.21 u turns.  With D = max |d_i|
                + eta: a square errs by 2 D eta + u D^2, the serial sum by (m - 1) u m D^2, the
                division by u V: the mean of squares by 2 D eta + (m + 3) u D^2.
                SE(3): the twist of E^-1 c_i moves with E by at most 2 (dphi + dt)(1 + |t_rel|)
                (rotations below one radian; dt the norm of the translation's error) and has
                its own arithmetic: the rotation part 44 u (the count of tests/test_policy_cpu.py),
                the translation part 7 u (the inverse's column) + 8 u (the product's) + 5 u (the
                V^-1 series): eta = 2 (dphi + dt)(1 + |t_rel|) + 64 u.
  variance      the distance from E to c_i errs by the matrix bound of tests/test_cluster_cpu.py,
                c u max(1, d) + 4 u pi (the wrapped terms' weights, per turn), c = W/2 + 3 (linked),
                5 (SE(2)), 5.5 + 44 w1 (SE(3)), and moves with E by at most the distance of the
                error itself: sqrt(sum (w_k dE_k)^2), w0 |dE_xy| + w1 dE_angle, w0 dt + w1 dphi.
                The mean of the squares then as for the variances.
  reached       a member whose distance to the target is closer to reached_distance than the
                matrix bound is not compared (none is, see test_reached_leaves_nothing_out).

The worst measured error / bound of every robot is printed (and recorded in DESIGN.md 4.19).

Each of these mutations of fks_summary.cpp / fks_rotation_mean.h fails the test named with it
(run against a mutated host build):
  the arithmetic mean for a continuous dof      test_members_straddling_pi
  division by n - 1                             test_hand_case_with_an_out_of_range_label
  the wrap dropped from the variance            test_members_straddling_pi
  an unstable regrouping                        test_regrouping_equals_the_restatement
  `<=` for reached                              test_reached_is_strict
  the eigenvector of the smallest eigenvalue    test_moments_against_high_precision[cfg4]
  the Jacobi iteration stopped after one sweep  test_moments_against_high_precision[cfg4]"""
import math

import numpy as np
import pytest

import cluster_cases as CC
import hp_policy
import hp_reference as hp
import hp_summary
from fast_kinematic_simulator_amd import _capi, cluster_outcomes_host, summarize_clusters_host

U = 2.0 ** -53
G40 = 1 + 2.0 ** -40
SIZES = (1, 2, 63, 64, 65, 256)
NAMES = CC.NAMES


def _c(robot):
    if robot.robot_type == _capi.ROBOT_LINKED:
        return robot.config_width / 2.0 + 3.0
    if robot.robot_type == _capi.ROBOT_SE2:
        return 5.0
    return 5.5 + 44.0 * float(robot.distance_weights[1])


def _distance_bound(robot, d, wraps):
    return (_c(robot) * U * max(1.0, float(d)) + 4 * U * math.pi * wraps) * G40


def _mean_of_squares_bound(m, largest, eta):
    D = largest + eta
    return (2 * D * eta + (m + 3) * U * D * D) * G40


def _expectation_bounds(robot, q, r):
    """(per entry of E its bound, dphi, dt) of one cluster r of hp_summary.moments on the group q"""
    m = len(r["members"])
    W = robot.config_width
    X = np.abs(q[r["members"]]).max(axis=0)
    bound = [m * U * float(X[k]) * G40 for k in range(W)]
    dphi = dt = 0.0
    for k, res in r["resultant"].items():
        e = math.sqrt(2.0) * m * U * (m + 1)
        bound[k] = (e / (float(res) - e) + 2 * U * math.pi) * G40
    if robot.robot_type == _capi.ROBOT_SE3:
        dS = 4 * m * U * (m + 20)
        dq = (2 * dS + 3840 * U * float(r["S_norm"])) / float(r["gap"]) + 2212 * U
        for i in range(3):
            for j in range(3):
                bound[4 * i + j] = (4 * dq + 4 * U) * G40
        dphi = (2 * dq + 8 * U) * G40
        dt = math.sqrt(sum(bound[4 * i + 3] ** 2 for i in range(3)))
    return bound, dphi, dt


def _spread_bounds(robot, r, bound_E, dphi, dt):
    """(per entry of the variances its bound, the scalar variance's bound)"""
    m = len(r["members"])
    diff = np.abs(hp.to_float(np.array(r["diff"], dtype=object)))
    turns = np.asarray(r["turns"], dtype=np.float64)
    Wv = diff.shape[1]
    if robot.robot_type == _capi.ROBOT_SE3:
        assert float(np.sqrt((diff[:, 3:] ** 2).sum(axis=1)).max()) < 1.0
        eta = [2 * (dphi + dt) * (1 + max(float(t) for t in r["trel"])) + 64 * U] * 6
        lip = float(robot.distance_weights[0]) * dt + float(robot.distance_weights[1]) * dphi
    else:
        raw = diff + 2 * math.pi * turns
        eta = [bound_E[k] + U * float(raw[:, k].max()) + 2.21 * U * float(turns[:, k].max()) for k in range(Wv)]
        w = [float(x) for x in robot.distance_weights]
        if robot.robot_type == _capi.ROBOT_LINKED:
            lip = math.sqrt(sum((w[k] * bound_E[k]) ** 2 for k in range(Wv)))
        else:
            lip = w[0] * math.hypot(bound_E[0], bound_E[1]) + w[1] * bound_E[2]
    variances = [_mean_of_squares_bound(m, float(diff[:, k].max()), eta[k]) for k in range(Wv)]
    dist = [float(d) for d in r["dist"]]
    eta_d = max(_distance_bound(robot, d, wr) for d, wr in zip(dist, r["dist_wraps"])) + lip
    return variances, _mean_of_squares_bound(m, max(dist), eta_d)


@pytest.fixture(scope="module")
def cases(fks_lib):
    """per robot: groups of the six sizes drawn in clumps, labelled by the twin's own clustering at
    a threshold between the clumps' diameter and their separation, one target (a clump's centre)
    per group, the twin's summary and the high-precision moments, computed once"""
    out = {}
    for seed, (name, robot) in enumerate(CC.robots().items()):
        rng = np.random.default_rng(900 + seed)
        groups, centres = [], None
        drawn, centres = CC.draw_clumped(robot, rng, sum(SIZES))
        at = 0
        for n in SIZES:
            groups.append(drawn[at:at + n])
            at += n
        D = cluster_outcomes_host(robot, [centres], 0.0, distances=True, labels=False)["distances"][0]
        mid = 0.5 * float(D[np.triu_indices(len(centres), 1)].min())
        labels = cluster_outcomes_host(robot, groups, mid)["labels"]
        targets = np.ascontiguousarray(centres[rng.integers(0, len(centres), len(SIZES))])
        twin = summarize_clusters_host(robot, groups, labels, targets=targets, reached_distance=mid)
        ref = [hp_summary.moments(robot, g, l) for g, l in zip(groups, labels)]
        out[name] = {"robot": robot, "groups": groups, "labels": labels, "targets": targets, "reach": mid, "twin": twin, "hp": ref}
    return out


@pytest.mark.parametrize("name", NAMES)
def test_regrouping_equals_the_restatement(cases, name):
    """order, members, count and begin, exactly"""
    case = cases[name]
    twin, at = case["twin"], 0
    for g, lab in zip(case["groups"], case["labels"]):
        n = len(lab)
        order, count, begin = hp_summary.regroup(lab)
        assert twin["order"][at:at + n].tolist() == [at + i for i in order]
        assert twin["count"][at:at + n].tolist() == count
        assert twin["begin"][at:at + n].tolist() == [at + b for b in begin]
        assert twin["members"][at:at + n].tobytes() == np.ascontiguousarray(g[order]).tobytes()
        if n >= 63:
            assert 2 <= sum(1 for c in count if c) <= 20 and max(count) >= 5, (name, n, count)
        at += n


@pytest.mark.parametrize("name", NAMES)
def test_moments_against_high_precision(cases, name):
    case = cases[name]
    robot, twin, B = case["robot"], case["twin"], hp.DEFAULT
    circ = set(hp_summary.circular_dims(robot))
    worst = {"expectation": 0.0, "variances": 0.0, "variance": 0.0}
    at = 0
    for g, ref in zip(case["groups"], case["hp"]):
        for c, r in enumerate(ref):
            row = at + c
            if r is None:
                assert twin["count"][row] == 0
                for key in ("expectation", "variances", "variance"):
                    assert np.all(np.atleast_1d(twin[key][row]).view(np.uint64) == 0), (name, key, "an empty cluster's row is +0.0")
                continue
            bound_E, dphi, dt = _expectation_bounds(robot, g, r)
            for k in range(robot.config_width):
                err = B.scalar(twin["expectation"][row][k]) - r["E"][k]
                err = abs(float(hp.wrap(err, B) if k in circ else err))  # angles are compared modulo a turn
                worst["expectation"] = max(worst["expectation"], err / bound_E[k])
            bound_V, bound_v = _spread_bounds(robot, r, bound_E, dphi, dt)
            for k in range(len(bound_V)):
                err = abs(float(B.scalar(twin["variances"][row][k]) - r["variances"][k]))
                worst["variances"] = max(worst["variances"], err / bound_V[k])
            err = abs(float(B.scalar(twin["variance"][row]) - r["variance"]))
            worst["variance"] = max(worst["variance"], err / bound_v)
        at += len(g)
    print(f"summary {name}: worst |error| / bound: expectation {worst['expectation']:.3f}, variances {worst['variances']:.3f}, "
          f"variance {worst['variance']:.3f}")
    assert max(worst.values()) <= 1.0, (name, worst)


@pytest.mark.parametrize("name", NAMES)
def test_reached_leaves_nothing_out(cases, name):
    """reached against the high-precision distances; the reach lies between the clumps, so no
    decision is nearer than its bound (at most 3 % may be)"""
    case = cases[name]
    robot, twin, B = case["robot"], case["twin"], hp.DEFAULT
    at, near, total, counted = 0, 0, 0, 0
    for gi, (g, lab) in enumerate(zip(case["groups"], case["labels"])):
        n = len(lab)
        q = B.array(g)
        t = list(B.array(case["targets"][gi]))
        want, sure = [0] * n, [True] * n
        for i in range(n):
            if int(lab[i]) >= n:
                continue
            d, wraps = hp_summary.distance(robot, B, list(q[i]), t)
            total += 1
            if abs(float(d) - case["reach"]) <= _distance_bound(robot, d, wraps):
                near += 1
                sure[int(lab[i])] = False
            elif float(d) < case["reach"]:
                want[int(lab[i])] += 1
        for c in range(n):
            if sure[c]:
                assert int(twin["reached"][at + c]) == want[c], (name, gi, c)
        counted += sum(want)
        at += n
    assert near == 0 and near <= 0.03 * total, (name, near, total)
    assert 0 < counted < total, (name, counted, total)


def test_both_backends_state_the_same_moments(cases):
    other = hp.Backend("mpmath" if hp.DEFAULT.kind == "longdouble" else "longdouble")
    if other.kind == "longdouble" and np.finfo(np.longdouble).eps >= 1e-18:
        pytest.skip("one backend on this platform: no 80-bit long double")
    for name, case in cases.items():
        for gi in (0, 1, 2):  # the groups of 1, 2 and 63
            b = hp_summary.moments(case["robot"], case["groups"][gi], case["labels"][gi], other)
            for ra, rb in zip(case["hp"][gi], b):
                assert (ra is None) == (rb is None)
                if ra is None:
                    continue
                # both backends round below 2^-63; what they share is float64's reading of it
                scale = 1.0 if case["robot"].robot_type != _capi.ROBOT_SE3 else max(1.0, float(rb["S_norm"]) / float(rb["gap"]))
                pairs = list(zip(ra["E"], rb["E"])) + list(zip(ra["variances"], rb["variances"])) + [(ra["variance"], rb["variance"])]
                for x, y in pairs:
                    assert abs(float(x) - float(y)) <= 2.0 ** -50 * abs(float(y)) + 1e-17 * scale, name


# ---------------------------------------------------------------- hand cases: everything is exact
def _hand(groups, labels, targets=None, reach=0.0):
    return summarize_clusters_host(CC.slider(), [np.asarray(g, dtype=np.float64).reshape(-1, 1) for g in groups], labels,
                                   targets=None if targets is None else np.asarray(targets, dtype=np.float64).reshape(-1, 1),
                                   reached_distance=reach)


def test_hand_case_with_an_out_of_range_label(fks_lib):
    """five members, labels [2, 0, 2, 9, 0]: label 9 is out of range and belongs to no cluster"""
    r = _hand([[1.0, 10.0, 3.0, 7.0, 20.0]], [[2, 0, 2, 9, 0]])
    assert r["order"].tolist() == [1, 4, 0, 2, 3]
    assert r["members"].reshape(-1).tolist() == [10.0, 20.0, 1.0, 3.0, 7.0]
    assert r["count"].tolist() == [2, 0, 2, 0, 0]
    assert r["begin"].tolist() == [0, 2, 2, 4, 4]
    assert r["expectation"].reshape(-1).tolist() == [15.0, 0.0, 2.0, 0.0, 0.0]
    # the population form: ((-5)^2 + 5^2) / 2 and ((-1)^2 + 1^2) / 2
    assert r["variances"].reshape(-1).tolist() == [25.0, 0.0, 1.0, 0.0, 0.0]
    assert r["variance"].tolist() == [25.0, 0.0, 1.0, 0.0, 0.0]
    for key in ("expectation", "variances", "variance"):
        assert np.all(r[key].reshape(-1)[[1, 3, 4]].view(np.uint64) == 0), "an empty cluster's doubles are +0.0"
    assert "reached" not in r


def test_non_dense_labels_and_a_second_group(fks_lib):
    """labels 5, 3, 5, 1 of six: clusters 1, 3 and 5 hold them, 0, 2 and 4 are empty; the second
    group's rows and positions start at its offset"""
    r = _hand([[4.0, 8.0, 6.0, 2.0, 9.0, 11.0], [100.0, 300.0]], [[5, 3, 5, 1, 5, 3], [1, 1]])
    assert r["order"].tolist() == [3, 1, 5, 0, 2, 4, 6, 7]
    assert r["count"].tolist() == [0, 1, 0, 2, 0, 3, 0, 2]
    assert r["begin"].tolist() == [0, 0, 1, 1, 3, 3, 6, 6]
    assert r["expectation"].reshape(-1).tolist() == [0.0, 2.0, 0.0, 9.5, 0.0, 19.0 / 3.0, 0.0, 200.0]
    assert r["variances"].reshape(-1)[[1, 3, 7]].tolist() == [0.0, 2.25, 10000.0]


def test_all_singletons_and_an_empty_group(fks_lib):
    r = _hand([[5.0, -2.0, 7.5], [], [1.0]], [[2, 1, 0], [], [0]])
    assert r["order"].tolist() == [2, 1, 0, 3]
    assert r["count"].tolist() == [1, 1, 1, 1] and r["begin"].tolist() == [0, 1, 2, 3]
    assert r["expectation"].reshape(-1).tolist() == [7.5, -2.0, 5.0, 1.0]
    assert r["variances"].reshape(-1).tolist() == [0.0] * 4 and r["variance"].tolist() == [0.0] * 4
    assert r["group_begin"].tolist() == [0, 3, 3, 4]
    empty = _hand([[]], [[]])
    assert empty["count"].tolist() == [] and empty["members"].shape == (0, 1)


def test_reached_is_strict(fks_lib):
    """distances 1, 0.5, 1 and 3 to the target 2 under reach 1: only the 0.5 counts; NaN never does"""
    r = _hand([[1.0, 2.5, 3.0, 5.0]], [[0, 0, 0, 1]], targets=[2.0], reach=1.0)
    assert r["reached"].tolist() == [1, 0, 0, 0]
    r = _hand([[1.0, 2.5, 3.0, 5.0]], [[0, 0, 0, 1]], targets=[2.0], reach=math.nextafter(1.0, 2.0))
    assert r["reached"].tolist() == [3, 0, 0, 0]
    r = _hand([[1.0, float("nan"), float("inf")]], [[0, 0, 0]], targets=[2.0], reach=float("inf"))
    assert r["reached"].tolist() == [1, 0, 0]


def test_members_straddling_pi(fks_lib):
    """a continuous dof with members 0.1 either side of the cut: the circular mean is at +-pi (the
    arithmetic mean would be 0) and the differences are wrapped (unwrapped: a whole turn less 0.1)"""
    robot = CC.workload("folding_arm_continuous").robot
    kinds = hp_policy.dof_kinds(robot)
    k = [i for i, kind in enumerate(kinds) if kind[0]][0]
    base = np.array([0.5 * (lo + hi) if not cont else 0.0 for cont, lo, hi in kinds])
    g = np.tile(base, (2, 1))
    g[0, k], g[1, k] = math.pi - 0.1, -math.pi + 0.1
    r = summarize_clusters_host(robot, [g], [[0, 0]])
    assert abs(abs(r["expectation"][0][k]) - math.pi) < 1e-15
    assert abs(r["variances"][0][k] - 0.01) < 1e-15
    others = [i for i in range(len(kinds)) if i != k]
    assert np.all(r["variances"][0][others] == 0.0) and np.array_equal(r["expectation"][0][others], base[others])
    w = float(robot.distance_weights[k])
    assert abs(r["variance"][0] - (w * 0.1) ** 2) < 1e-15
