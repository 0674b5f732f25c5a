"""Robots and scenes with the joint types, axes and origins the BASELINE workloads never have:
prismatic and continuous joints, oblique and non-unit axes, rotated joint origins, a branched
tree, and a serial chain wider than the 8x8 least-squares tile.  Test helper (not a workload of
the product): tests/test_joint_zoo_cpu.py holds the oracle on these robots to a high-precision
reference, tests/test_joint_zoo.py holds the HIP path to both.

Every scene runs in the open-space environment (a floor slab under the robot) at 50 Hz for
1 s of simulated time."""
import numpy as np

from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd.robots import ControllerConfig, Joint, make_linked_robot, rotation_from_axis_angle, transform34
from fast_kinematic_simulator_amd.simulator import SimulatorSolverParameters
from fast_kinematic_simulator_amd.workloads import Workload, _open_space_env, cylinder_points

REV, CONT, PRIS, FIXED = _capi.JOINT_REVOLUTE, _capi.JOINT_CONTINUOUS, _capi.JOINT_PRISMATIC, _capi.JOINT_FIXED


def _controllers(d, vmax=1.0):
    return [ControllerConfig(kp=10.0, ki=1.0, kd=0.1, integral_clamp=0.5, velocity_limit=vmax, acceleration_limit=vmax * 10,
                             max_actuator_proportional_noise=0.2, max_actuator_minimum_noise=0.0002) for _ in range(d)]


def _workload(name, description, robot, starts, target, seed):
    solver = SimulatorSolverParameters(forward_simulation_time=1.0)
    return Workload(name, description, robot, _open_space_env, np.asarray(starts, dtype=np.float64),
                    np.asarray(target, dtype=np.float64).reshape(1, -1), solver, 50.0, seed, True, 128, 0.01)


# ---------------------------------------------------------------- mixed_tree
OBLIQUE_ORIGIN = rotation_from_axis_angle([0.36, 0.48, 0.8], 0.7)


def mixed_tree_robot(skew=False):
    """7 links, 5 dofs, 256 points.  base -> 1 revolute about z; 1 -> 2 prismatic along (2, -3, -6) / 7
    behind a rotated origin; 2 -> 3 fixed behind the same rotated origin; 3 -> 4 continuous about
    (0.6, 0, 0.8); the branch 1 -> 5 revolute about (1, 2, 2) / 3 and 5 -> 6 prismatic along z with
    asymmetric limits.  skew=True scales the branch's revolute axis to norm 1.5 (an AngleAxis that is
    no rotation: the skip proofs have no lever for it)."""
    branch_axis = np.array([1.0, 2.0, 2.0]) / 3.0 * (1.5 if skew else 1.0)
    joints = [
        Joint(0, 1, REV, transform34([0.0, 0.0, 0.10]), (0.0, 0.0, 1.0), -2.9, 2.9),
        Joint(1, 2, PRIS, transform34([0.0, 0.0, 0.22], OBLIQUE_ORIGIN), (2.0 / 7.0, -3.0 / 7.0, -6.0 / 7.0), -0.35, 0.35),
        Joint(2, 3, FIXED, transform34([0.0, 0.0, 0.12], OBLIQUE_ORIGIN)),
        Joint(3, 4, CONT, transform34([0.0, 0.0, 0.04]), (0.6, 0.0, 0.8), -np.pi, np.pi),
        Joint(1, 5, REV, transform34([0.05, 0.0, 0.12], rotation_from_axis_angle([0.0, 1.0, 0.0], 0.9)), tuple(branch_axis), -2.0, 2.0),
        Joint(5, 6, PRIS, transform34([0.0, 0.0, 0.16]), (0.0, 0.0, 1.0), -0.05, 0.3),
    ]
    geoms = [(0, cylinder_points(0.10, 0.05, 64, 16)),
             (1, cylinder_points(0.20, 0.035, 48, 12)),
             (2, cylinder_points(0.12, 0.03, 32, 8)),
             (4, cylinder_points(0.18, 0.025, 48, 12)),
             (5, cylinder_points(0.16, 0.03, 32, 8)),
             (6, cylinder_points(0.14, 0.02, 32, 8))]
    # geometry indices: 0 base, 1 link 1, 2 link 2, 3 link 4, 4 link 5, 5 link 6
    allowed = [(a, b) for a in range(6) for b in range(a + 1, 6)]  # every pair: telescope has the self-collisions
    return make_linked_robot(transform34([0.0, 0.0, -0.10]), 7, joints, geoms, allowed, _controllers(5), [1.0] * 5,
                             name="mixed_tree_skew" if skew else "mixed_tree")


MIXED_NOMINAL = np.array([0.0, 0.0, 2.9, 0.3, 0.0])
MIXED_TARGET = np.array([0.8, 0.34, -2.9, 1.2, 0.28])


def mixed_tree(n=16, skew=False):
    robot = mixed_tree_robot(skew)
    rng = np.random.default_rng(31)
    starts = MIXED_NOMINAL + rng.uniform(-0.03, 0.03, size=(n, 5))
    return _workload("skew_axis" if skew else "mixed_tree", "branched tree of revolute, prismatic, fixed and continuous joints",
                     robot, starts, MIXED_TARGET, 31)


def skew_axis(n=16):
    return mixed_tree(n, skew=True)


# ---------------------------------------------------------------- gantry
def gantry_robot():
    """Four prismatic dofs: x and y with unit axes, z with the axis (0, 0, 2) (motion is axis * q,
    not normalised), and a fourth joint parallel to the first, so its Jacobian column equals the
    first dof's bit for bit: a pivot tie and a rank-deficient system in every solve.  The last link
    carries the tool."""
    joints = [
        Joint(0, 1, PRIS, transform34([0.0, 0.0, 0.30]), (1.0, 0.0, 0.0), -0.3, 0.3),
        Joint(1, 2, PRIS, transform34([0.0, 0.0, 0.02]), (0.0, 1.0, 0.0), -0.3, 0.3),
        Joint(2, 3, PRIS, transform34([0.0, 0.0, -0.02]), (0.0, 0.0, 2.0), -0.2, 0.05),
        Joint(3, 4, PRIS, transform34([0.0, 0.0, -0.04]), (1.0, 0.0, 0.0), -0.1, 0.1),
    ]
    bar = cylinder_points(0.2, 0.015, 32, 8, z0=-0.1)
    geoms = [(1, bar[:, [2, 0, 1, 3]]),                      # the x carriage's bar, along x
             (2, bar[:, [0, 2, 1, 3]]),                      # the y carriage's bar, along y
             (3, cylinder_points(0.04, 0.02, 32, 8, z0=-0.04)),
             (4, cylinder_points(0.10, 0.015, 64, 16, z0=-0.10))]  # the tool, pointing down
    allowed = [(0, 1), (1, 2), (2, 3), (0, 2), (1, 3), (0, 3)]  # carriages slide through each other
    return make_linked_robot(transform34([0.0, 0.0, 0.0]), 5, joints, geoms, allowed, _controllers(4, vmax=0.5), [1.0] * 4,
                             name="gantry")


GANTRY_TARGET = np.array([0.2, -0.15, -0.19, 0.05])


def gantry(n=16):
    robot = gantry_robot()
    rng = np.random.default_rng(32)
    starts = np.array([0.0, 0.0, 0.0, 0.0]) + rng.uniform(-0.02, 0.02, size=(n, 4))
    starts[0, 2] = 0.4  # a prismatic start outside its limits [-0.2, 0.05]: ResetPosition clamps it
    return _workload("gantry", "four prismatic dofs, two of them parallel, a tool driven into the floor", robot, starts,
                     GANTRY_TARGET, 32)


# ---------------------------------------------------------------- telescope
def telescope_robot():
    """revolute, prismatic, revolute: the prismatic link retracts along the upper arm into the base
    column, a link it is not adjacent to and may not touch."""
    joints = [
        Joint(0, 1, REV, transform34([0.0, 0.0, 0.10]), (0.0, 1.0, 0.0), -2.5, 2.5),
        Joint(1, 2, PRIS, transform34([0.0, 0.0, 0.05]), (0.0, 0.0, 1.0), -0.2, 0.2),
        Joint(2, 3, REV, transform34([0.0, 0.0, 0.20]), (0.6, 0.8, 0.0), -2.5, 2.5),
    ]
    geoms = [(0, cylinder_points(0.10, 0.05, 64, 16)),
             (1, cylinder_points(0.05, 0.04, 32, 8)),
             (2, cylinder_points(0.20, 0.02, 64, 16)),
             (3, cylinder_points(0.15, 0.02, 32, 8))]
    allowed = [(0, 1), (1, 2), (2, 3)]
    return make_linked_robot(transform34([0.0, 0.0, 0.0]), 4, joints, geoms, allowed, _controllers(3), [1.0] * 3, name="telescope")


TELESCOPE_TARGET = np.array([0.3, -0.19, 0.8])


def telescope(n=16):
    robot = telescope_robot()
    rng = np.random.default_rng(33)
    starts = np.array([0.0, 0.1, 0.2]) + rng.uniform(-0.03, 0.03, size=(n, 3))
    return _workload("telescope", "a prismatic link retracting into a non-adjacent link (self-collision)", robot, starts,
                     TELESCOPE_TARGET, 33)


# ---------------------------------------------------------------- wide_mixed
def wide_mixed_robot():
    """A 10-dof serial chain alternating revolute joints about oblique unit axes with short-stroke
    prismatic joints: wider than the 8x8 tile, so the column-per-lane solver runs."""
    axes = [(0.0, 0.6, 0.8), (2.0 / 3.0, -1.0 / 3.0, 2.0 / 3.0), (3.0 / 13.0, 4.0 / 13.0, 12.0 / 13.0), (0.8, 0.0, -0.6),
            (6.0 / 7.0, 2.0 / 7.0, 3.0 / 7.0)]
    slides = [(0.0, 0.0, 1.0), (0.28, 0.0, 0.96), (0.0, 0.0, 1.0), (0.0, -0.6, 0.8), (0.0, 0.0, 1.0)]
    joints, geoms = [], [(0, cylinder_points(0.06, 0.04, 16, 4))]
    tilt = rotation_from_axis_angle([1.0, 1.0, 0.0], 0.3)
    for i in range(10):
        if i % 2 == 0:
            joints.append(Joint(i, i + 1, REV, transform34([0.0, 0.0, 0.06], tilt if i % 4 == 0 else None), axes[i // 2], -2.0, 2.0))
        else:
            joints.append(Joint(i, i + 1, PRIS, transform34([0.0, 0.0, 0.05]), slides[i // 2], -0.02, 0.04))
        geoms.append((i + 1, cylinder_points(0.05, 0.015, 16, 4)))
    allowed = [(i, i + 1) for i in range(10)] + [(i, i + 2) for i in range(9)]
    return make_linked_robot(transform34([0.0, 0.0, 0.42], rotation_from_axis_angle([0.0, 1.0, 0.0], 2.3)), 11, joints, geoms, allowed, _controllers(10), [1.0] * 10, name="wide_mixed")


WIDE_TARGET = np.array([-0.9, 0.035, -1.0, 0.035, -0.8, 0.035, -0.7, 0.035, -0.5, 0.035])


def wide_mixed(n=16):
    robot = wide_mixed_robot()
    rng = np.random.default_rng(34)
    starts = np.tile([0.1, 0.0], 5) + rng.uniform(-0.02, 0.02, size=(n, 10)) * np.tile([1.0, 0.5], 5)
    return _workload("wide_mixed", "10-dof chain of oblique revolute and short prismatic joints", robot, starts, WIDE_TARGET, 34)


SCENES = {"mixed_tree": mixed_tree, "gantry": gantry, "telescope": telescope, "wide_mixed": wide_mixed, "skew_axis": skew_axis}
MEASURABLE = ("mixed_tree", "gantry", "telescope", "wide_mixed")  # skew_axis: a non-unit AngleAxis is no rotation


def check_scene(name, wl, r):
    """The conditions a run of the scene must meet for its parity to mean anything (the branch was
    reached); `r` is a result dict of the oracle or of the HIP path."""
    c = r["counters"]
    assert not np.any(r["error_flags"]), np.unique(r["error_flags"])
    assert c["resolver_iterations"] > 0, c
    assert r["collided"].any()
    q = r["positions"]
    if name in ("mixed_tree", "skew_axis"):
        # the continuous dof starts near +2.9 and is sent to -2.9: it went through +-pi
        assert np.any(np.sign(q[:, 2]) == -np.sign(wl.starts[:, 2])), q[:, 2]
    if name == "gantry":
        # the z slide (dof 2) stopped strictly inside its limits and short of its target: a contact
        # stopped it, not the clamp
        lo, hi = wl.robot.dof_limits()
        z, zt = q[:, 2], wl.targets[0, 2]
        assert np.any((z > lo[2]) & (z < hi[2]) & (z > zt + 0.01)), z
    if name == "telescope":
        assert c["self_corrected_points"] > 0, c
    if name == "wide_mixed":
        assert c["least_squares_rows"] > 0, c
