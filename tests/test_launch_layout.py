"""The launch layout fks_set_robot chooses, field by field, against a recording of the commit
before csrc/fks_launch.cpp took the decision over (tests/golden/launch_layouts.json): the robots
of cfg1-cfg5 and of the joint zoo in the joint zoo's open-space environment.  Nothing is simulated.

The fixture holds the resident figures per CU, so a device in another partition mode (fewer CUs)
compares too; a figure that does not divide by the CU count means the HBM cap engaged, which the
fixture's robots never reach on an MI355X."""
import json
import os

import pytest

import joint_zoo as Z
from fast_kinematic_simulator_amd import make_linked_simulator, workloads

DEVICE = 0  # of the context and of the CU count alike
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_layouts.json")
RESIDENT = ("resident_waves", "small_batch_resident_waves", "standard_layout_resident_waves", "cooperative_resident_particles")
ZOO_ROBOTS = {"mixed_tree": Z.mixed_tree_robot, "gantry": Z.gantry_robot, "telescope": Z.telescope_robot,
              "wide_mixed": Z.wide_mixed_robot, "skew_axis": lambda: Z.mixed_tree_robot(skew=True)}
NAMES = tuple(workloads.WORKLOADS) + tuple(ZOO_ROBOTS)


def robot_of(name):
    if name in ZOO_ROBOTS:
        return ZOO_ROBOTS[name]()
    return workloads.WORKLOADS[name](scale=1.0 / (1 << 20)).robot  # one particle: only the robot is used


def compute_units():
    import torch

    return int(torch.cuda.get_device_properties(DEVICE).multi_processor_count)


def layouts(names=NAMES):
    """launch_info() after set_robot for each named robot, on one simulator"""
    wl = Z.gantry(1)
    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed, device=DEVICE)
    try:
        out = {}
        for name in names:
            sim.set_robot(robot_of(name))
            out[name] = sim.launch_info()
        return out
    finally:
        sim.close()


def per_cu(info, cus):
    """the resident figures divided by the CU count; each must divide evenly"""
    out = dict(info)
    for k in RESIDENT:
        assert info[k] % cus == 0, (k, info[k], cus, "the HBM cap engaged")
        out[k] = info[k] // cus
    return out


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def measured(fks_lib):
    return layouts()


@pytest.mark.parametrize("name", NAMES)
def test_layout_equals_recording(measured, name):
    golden = json.load(open(GOLDEN))
    assert per_cu(measured[name], compute_units()) == golden[name]
