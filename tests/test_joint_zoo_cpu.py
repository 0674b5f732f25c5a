"""The CPU oracle held to mathematics on the joint zoo (tests/joint_zoo.py): prismatic and
continuous joints, oblique and non-unit axes, rotated origins, a branched tree.

Bit parity between the HIP path and the oracle shows that both compute the same thing; much of
that arithmetic is written once and compiled for both sides, so parity cannot show that it is
right.  Here the oracle's forward kinematics, world points, point Jacobians and clean
ApplyControlInput are compared with tests/hp_reference.py (80-bit or 40-digit arithmetic written
from the definitions), for the four measurable zoo robots and for the SE(2) and SE(3) robots of
cfg1 and cfg4.

Tolerance per element (linked robots): 16 (n + 1) 2^-53 max(1, reach), n the joints on the link's
path and reach the sum of the path's origin translations, prismatic strokes and the point's
norm.  A joint costs two 3x4 compositions of about a dozen rounded operations each on values
bounded by reach, plus a sine and cosine within 1 ulp; the + 1 is the point's own transform.
Each test prints the worst observed ratio to its bound (DESIGN.md §3 records them).

The non-vacuity tests show on the oracle alone that every zoo scene reaches what it is for."""
import functools

import numpy as np
import pytest

import hp_reference as H
import joint_zoo as Z
from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd import workloads as W

U = 2.0 ** -53


def xform(T, p):
    """3x4 transform of 4-vectors in the canonical order (r0*p0 + r1*p1) + r2*p2 + t*w."""
    out = np.empty((len(p), 3))
    for r in range(3):
        out[:, r] = ((T[4 * r] * p[:, 0] + T[4 * r + 1] * p[:, 1]) + T[4 * r + 2] * p[:, 2]) + T[4 * r + 3] * p[:, 3]
    return out


@functools.lru_cache(maxsize=None)
def zoo_robot(name):
    return Z.SCENES[name]().robot


def zoo_configs(robot, n=20, seed=41):
    """n seeded configurations inside the limits; the first four: every dof at its lower limit, at
    its upper limit (continuous dofs: -pi and +pi), and the continuous dofs alone at -pi and +pi."""
    lo, hi = robot.dof_limits()
    rng = np.random.default_rng(seed)
    q = rng.uniform(lo, hi, size=(n, len(lo)))
    q[0], q[1] = lo, hi
    cont = [k for k, j in enumerate(j for j in robot.joints if j.type != _capi.JOINT_FIXED) if j.type == _capi.JOINT_CONTINUOUS]
    for k in cont:
        q[2, k], q[3, k] = -np.pi, np.pi
    return q


def link_tolerance(robot, link, point=None):
    return 16.0 * (len(H.link_path(robot, link)) + 1) * U * max(1.0, H.reach(robot, link, point))


def sample_points(robot, g):
    pts = np.asarray(robot.geometry_points[g])
    return pts[[0, len(pts) // 2, len(pts) - 1]]


def moving_joints(robot):
    """(dof, joint) of every moving joint; joint_index_of_dof() gives its place in robot.joints"""
    return [(k, j) for k, j in enumerate(j for j in robot.joints if j.type != _capi.JOINT_FIXED)]


def joint_index_of_dof(robot):
    return [i for i, j in enumerate(robot.joints) if j.type != _capi.JOINT_FIXED]


def kinematics_ratios(robot, q, transforms, points):
    """Worst |value - hp| / tolerance of the link transforms (per geometry, 12 values) and of the world
    points (P, 3) of one configuration."""
    T = H.link_transforms(robot, q)
    worst_t = worst_p = 0.0
    at = 0
    for g, link in enumerate(robot.geometry_link):
        worst_t = max(worst_t, H.max_abs_diff(T[link][:3, :].reshape(12), transforms[g]) / link_tolerance(robot, link))
        pts = np.asarray(robot.geometry_points[g])
        hp = (H.DEFAULT.array(pts) @ T[link].T)[:, :3]
        d = np.abs(H.to_float(hp - H.DEFAULT.array(points[at:at + len(pts)])))
        tol = np.array([link_tolerance(robot, link, p) for p in pts])
        worst_p = max(worst_p, float(np.max(d / tol[:, None])))
        at += len(pts)
    return worst_t, worst_p


# ---------------------------------------------------------------- the reference itself
def test_reference_backends_agree():
    """The long-double and the 40-digit backends run the same code: they agree to long-double
    rounding on a robot with every joint type."""
    robot = zoo_robot("mixed_tree")
    q = zoo_configs(robot, 6)[5]
    mp = H.Backend("mpmath")
    a = H.world_points(robot, q)
    b = H.world_points(robot, q, mp)

    def exact(y):  # a backend value as an mpf: high part + low part, both float64, exactly
        return mp.mp.mpf(float(y)) + mp.mp.mpf(float(y - H.DEFAULT.scalar(float(y))))

    assert max(abs(float(x - exact(y))) for x, y in zip(b.reshape(-1), a.reshape(-1))) < 1e-17
    Ja = H.to_float(H.point_jacobian(robot, q, 3, robot.geometry_points[3][5]))
    Jb = H.to_float(H.point_jacobian(robot, q, 3, robot.geometry_points[3][5], mp))
    assert np.max(np.abs(Ja - Jb)) < 4 * U


@pytest.mark.parametrize("name", Z.MEASURABLE)
def test_reference_jacobian_is_the_derivative_of_its_fk(name):
    """The reference's Jacobian against central differences of the reference's own world point, both
    in high precision (h = 1e-6: truncation ~1e-12, rounding ~1e-13)."""
    robot = zoo_robot(name)
    q = zoo_configs(robot, 8)[7]
    lo, hi = robot.dof_limits()
    q = np.clip(q, lo + 1e-3, hi - 1e-3)
    g = len(robot.geometry_points) - 1
    p = np.asarray(robot.geometry_points[g][3])
    link = robot.geometry_link[g]
    J = H.point_jacobian(robot, q, g, p)
    h = H.DEFAULT.scalar(1e-6)
    for k in range(robot.num_dofs):
        qp, qm = list(H.DEFAULT.array(q)), list(H.DEFAULT.array(q))
        qp[k], qm[k] = qp[k] + h, qm[k] - h
        xp = (H.link_transforms(robot, qp)[link] @ H.DEFAULT.array(p))[:3]
        xm = (H.link_transforms(robot, qm)[link] @ H.DEFAULT.array(p))[:3]
        assert np.max(np.abs(H.to_float((xp - xm) / (2 * h) - J[:, k]))) < 1e-10, (name, k)


# ---------------------------------------------------------------- linked robots: FK, points, Jacobians
@pytest.mark.parametrize("name", Z.MEASURABLE)
def test_oracle_fk_and_points_match_reference(oracle_lib, name):
    import oracle

    robot = zoo_robot(name)
    worst_t = worst_p = 0.0
    for q in zoo_configs(robot):
        To = oracle.link_transforms(robot, q)
        world = np.concatenate([xform(To[g], np.asarray(robot.geometry_points[g])) for g in range(len(To))], axis=0)
        rt, rp = kinematics_ratios(robot, q, To, world)
        worst_t, worst_p = max(worst_t, rt), max(worst_p, rp)
    print(f"{name}: worst ratio to the bound: link transforms {worst_t:.3f}, world points {worst_p:.3f}")
    assert worst_t <= 1.0 and worst_p <= 1.0


@pytest.mark.parametrize("name", Z.MEASURABLE)
def test_oracle_jacobian_matches_reference(oracle_lib, name):
    import oracle

    robot = zoo_robot(name)
    dofs = moving_joints(robot)
    worst = 0.0
    prismatic_seen = revolute_seen = off_path_seen = 0
    for q in zoo_configs(robot):
        To = oracle.link_transforms(robot, q)
        geometry_of_link = {link: g for g, link in enumerate(robot.geometry_link)}
        for g, link in enumerate(robot.geometry_link):
            path = set(H.link_path(robot, link))
            on_path = [k for k, i in enumerate(joint_index_of_dof(robot)) if i in path]
            for p in sample_points(robot, g):
                J = oracle.point_jacobian(robot, q, g, p)
                ref = H.point_jacobian(robot, q, g, p)
                tol = link_tolerance(robot, link, p)
                worst = max(worst, float(np.max(np.abs(H.to_float(ref - H.DEFAULT.array(J))))) / tol)
                for k, j in dofs:
                    if k not in on_path:
                        assert np.all(J[:, k] == 0.0) and not np.any(np.signbit(J[:, k])), (name, g, k)
                        off_path_seen += 1
                    elif j.type == _capi.JOINT_PRISMATIC:
                        # the world axis: the joint frame's rotation applied to the axis as given
                        Tc = To[geometry_of_link[j.child]]
                        a = np.asarray(j.axis, dtype=np.float64)
                        axis_w = np.array([(Tc[4 * r] * a[0] + Tc[4 * r + 1] * a[1]) + Tc[4 * r + 2] * a[2] for r in range(3)])
                        assert np.array_equal(J[:, k], axis_w), (name, g, k, J[:, k], axis_w)
                        prismatic_seen += 1
                    else:
                        revolute_seen += 1
    print(f"{name}: worst ratio to the bound: point Jacobians {worst:.3f}")
    assert worst <= 1.0
    assert prismatic_seen > 0 and (revolute_seen > 0 or name == "gantry") and (off_path_seen > 0 or name != "mixed_tree")


def test_parallel_gantry_columns_are_bit_equal(oracle_lib):
    import oracle

    robot = zoo_robot("gantry")
    tool = len(robot.geometry_points) - 1
    for q in zoo_configs(robot, 6):
        for p in sample_points(robot, tool):
            J = oracle.point_jacobian(robot, q, tool, p)
            assert J[:, 0].tobytes() == J[:, 3].tobytes()
            assert np.array_equal(J[:, 0], [1.0, 0.0, 0.0]) and np.array_equal(J[:, 2], [0.0, 0.0, 2.0])  # axis * q, not normalised


def test_set_position_clamps_a_start_outside_the_limits(oracle_lib):
    """ResetPosition -> SetPosition clamps a prismatic value outside its limits (the lever arms of the
    skip proofs rely on it): the zoo's gantry has such a start."""
    import oracle

    wl = Z.gantry()
    lo, hi = wl.robot.dof_limits()
    q = wl.starts[0]
    assert q[2] > hi[2]
    clamped = np.clip(q, lo, hi)
    assert np.array_equal(oracle.link_transforms(wl.robot, q), oracle.link_transforms(wl.robot, clamped))
    assert np.array_equal(oracle.apply_control_input(wl.robot, q, np.zeros(4)), clamped)


# ---------------------------------------------------------------- ApplyControlInput
def control_cases(robot, n=24, seed=43):
    """configurations inside the limits and inputs that cross the joint limits, the +-pi cut and (in a
    quarter of the rows) the actuators' velocity limits"""
    rng = np.random.default_rng(seed)
    q = zoo_configs(robot, n, seed)
    vmax = np.array([abs(c.velocity_limit) for c in robot.controllers])
    u = rng.uniform(-0.9, 0.9, size=q.shape) * vmax
    u[::4] = rng.uniform(-1.8, 1.8, size=u[::4].shape) * vmax
    return q, u, vmax


def check_apply_control_input(robot, q, u, vmax, outputs, who):
    """The assertions on clean ApplyControlInput results `outputs` (one row per row of q, u), whoever
    computed them.  TNUVA:538-566 decide the exact expression: the input first goes through the
    actuator (GetControlValue, TNUVA:556: a clamp to +-velocity_limit), the sum q + u is rounded once
    (TNUVA:558), CopyWithNewValue enforces the limits (TNUVA:559) and SetPosition enforces them again
    (DESIGN §2.2), which changes nothing: a clamp and a wrap are idempotent.  So non-continuous dofs
    are exactly clamp(q + clamp(u, +-vmax), lo, hi) in float64, and continuous dofs lie within
    4 2^-53 pi of the high-precision wrap of the exact sum (the rounding of a sum below 8, the
    float64 2 pi and the final subtraction).  Returns the worst ratio to that bound."""
    lo, hi = robot.dof_limits()
    dofs = moving_joints(robot)
    clamped = wrapped = limited = 0
    worst = 0.0
    for qi, ui, out in zip(q, u, outputs):
        ref = H.apply_control_input(robot, qi, ui)
        raw = qi + np.clip(ui, -vmax, vmax)
        limited += int(np.sum(np.abs(ui) > vmax))
        for k, j in dofs:
            if j.type == _capi.JOINT_CONTINUOUS:
                err = abs(float(ref[k] - H.DEFAULT.scalar(out[k])))
                worst = max(worst, err / (4 * U * np.pi))
                assert -np.pi <= out[k] <= np.pi
                wrapped += int(abs(raw[k]) > np.pi)
            else:
                assert out[k] == min(max(raw[k], lo[k]), hi[k]), (who, k, qi[k], ui[k], out[k])
                assert abs(float(ref[k]) - out[k]) <= 2 * U * max(1.0, abs(raw[k]))  # the reference's sum is unrounded
                clamped += int(raw[k] < lo[k] or raw[k] > hi[k])
    print(f"{who}: worst ratio to the bound: continuous wrap {worst:.3f}")
    assert worst <= 1.0
    assert clamped > 0 and limited > 0
    assert wrapped > 0 or not any(j.type == _capi.JOINT_CONTINUOUS for _, j in dofs)
    return worst


@pytest.mark.parametrize("name", Z.MEASURABLE)
def test_oracle_apply_control_input(oracle_lib, name):
    import oracle

    robot = zoo_robot(name)
    q, u, vmax = control_cases(robot)
    check_apply_control_input(robot, q, u, vmax, [oracle.apply_control_input(robot, qi, ui) for qi, ui in zip(q, u)], name)


# ---------------------------------------------------------------- SE(2), SE(3)
def se2_cases():
    wl = W.cfg1(0.25)
    q = np.concatenate([wl.starts, wl.starts[:2]], axis=0)
    q[-2, 2], q[-1, 2] = np.pi, -np.pi
    return wl.robot, q


def se3_cases():
    wl = W.cfg4(8 / 1048576)
    return wl.robot, wl.starts


def test_se2_matches_reference(oracle_lib):
    """One rotation and one point transform: the linked bound with one joint, reach |t| + |p|.  The
    Jacobian is [e_x, e_y, e_z x (x - p)]: its third column carries the rounding of x."""
    import oracle

    robot, configs = se2_cases()
    pts = np.asarray(robot.geometry_points[0])
    rng = np.random.default_rng(47)
    vmax = np.array([abs(c.velocity_limit) for c in robot.controllers])
    worst = {"fk": 0.0, "points": 0.0, "jacobian": 0.0, "wrap": 0.0}
    for q in configs:
        scale = 16.0 * 2 * U * max(1.0, float(np.hypot(q[0], q[1])) + float(np.max(np.linalg.norm(pts[:, :3], axis=1))))
        To = oracle.link_transforms(robot, q)[0]
        T = H.se2_transform(q)
        worst["fk"] = max(worst["fk"], H.max_abs_diff(T[:3, :].reshape(12), To) / scale)
        hp = (H.DEFAULT.array(pts) @ T.T)[:, :3]
        worst["points"] = max(worst["points"], H.max_abs_diff(hp, xform(To, pts)) / scale)
        for p in pts[[0, 27, 63]]:
            J = oracle.point_jacobian(robot, q, 0, p)
            assert np.array_equal(J[:, :2], [[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]) and J[2, 2] == 0.0
            worst["jacobian"] = max(worst["jacobian"], H.max_abs_diff(H.se2_jacobian(q, p), J) / scale)
        u = rng.uniform(-1.5, 1.5, size=3) * vmax
        u[2] = np.copysign(vmax[2], q[2]) if abs(q[2]) > 2.7 else u[2]  # over the cut where the start is near it
        out = oracle.apply_control_input(robot, q, u)
        ref = H.apply_control_input(robot, q, u)
        v = np.clip(u, -vmax, vmax)
        assert out[0] == q[0] + v[0] and out[1] == q[1] + v[1]
        worst["wrap"] = max(worst["wrap"], abs(float(ref[2] - H.DEFAULT.scalar(out[2]))) / (4 * U * np.pi))
    print("se2: worst ratio to the bound:", ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def test_se3_matches_reference(oracle_lib):
    """The configuration is the pose: the link transform is a copy (exact).  A point costs one 3x4
    transform (n = 0).  The rotational Jacobian columns (R e_k) x (x - t) carry x's rounding and a
    cross product (n = 1).  ApplyControlInput is P exp(twist): the exponential (a sine, a square root
    and about thirty operations) and one composition, counted as two joints (n = 2), reach |t| + |v|."""
    import oracle

    robot, configs = se3_cases()
    pts = np.asarray(robot.geometry_points[0])
    rmax = float(np.max(np.linalg.norm(pts[:, :3], axis=1)))
    rng = np.random.default_rng(53)
    vmax = np.array([abs(c.velocity_limit) for c in robot.controllers])
    worst = {"points": 0.0, "jacobian": 0.0, "apply": 0.0}
    for i, P in enumerate(configs):
        t = float(np.linalg.norm(P[[3, 7, 11]]))
        To = oracle.link_transforms(robot, P)[0]
        assert np.array_equal(To, P)
        hp = (H.DEFAULT.array(pts) @ H.from34(P).T)[:, :3]
        worst["points"] = max(worst["points"], H.max_abs_diff(hp, xform(To, pts)) / (16.0 * U * max(1.0, t + rmax)))
        for p in pts[[0, 100, 255]]:
            J = oracle.point_jacobian(robot, P, 0, p)
            worst["jacobian"] = max(worst["jacobian"], H.max_abs_diff(H.se3_jacobian(P, p), J) / (16.0 * 2 * U * max(1.0, t + rmax)))
        # twists from 1e-6 of the limits (the series of the exponential's coefficients) to past them
        u = rng.uniform(-1.0, 1.0, size=6) * vmax * (1e-6, 1e-3, 0.05, 0.3, 1.0, 1.0, 1.6, 1.6)[i % 8]
        out = oracle.apply_control_input(robot, P, u)
        v = np.clip(u, -vmax, vmax)
        ref = H.apply_control_input(robot, P, u)
        worst["apply"] = max(worst["apply"], H.max_abs_diff(ref, out) / (16.0 * 3 * U * max(1.0, t + float(np.linalg.norm(v[:3])))))
    print("se3: worst ratio to the bound:", ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def test_reference_se3_jacobian_is_the_derivative_of_the_exponential():
    """Body-twist columns: d/d eps of P exp(eps e_k) x at eps = 0, by central differences of the
    reference's closed-form exponential in high precision; the same for SE(2)'s additive columns."""
    robot, configs = se3_cases()
    P = configs[3]
    p = np.asarray(robot.geometry_points[0][17])
    B = H.DEFAULT
    J = H.se3_jacobian(P, p)
    h = B.scalar(1e-6)
    for k in range(6):
        e = B.zeros(6)
        e[k] = h
        xp = (H.from34(P) @ H.se3_exp(e) @ B.array(p))[:3]
        xm = (H.from34(P) @ H.se3_exp(-e) @ B.array(p))[:3]
        assert np.max(np.abs(H.to_float((xp - xm) / (2 * h) - J[:, k]))) < 1e-10, k
    robot2, configs2 = se2_cases()
    q = configs2[1]
    p2 = np.asarray(robot2.geometry_points[0][9])
    J2 = H.se2_jacobian(q, p2)
    for k in range(3):
        qp, qm = list(B.array(q)), list(B.array(q))
        qp[k], qm[k] = qp[k] + h, qm[k] - h
        d = ((H.se2_transform(qp) @ B.array(p2))[:3] - (H.se2_transform(qm) @ B.array(p2))[:3]) / (2 * h)
        assert np.max(np.abs(H.to_float(d - J2[:, k]))) < 1e-10, k


# ---------------------------------------------------------------- the scenes reach what they are for
@pytest.mark.parametrize("name", sorted(Z.SCENES))
def test_oracle_zoo_scene_reaches_branch(oracle_lib, name):
    import oracle

    wl = Z.SCENES[name]()
    o = oracle.forward_simulate(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, wl.starts, wl.targets, True)
    Z.check_scene(name, wl, o)
    print(name, {k: o["counters"][k] for k in ("microsteps", "resolver_iterations", "least_squares_rows", "self_corrected_points")})
