"""The path-job entries without a GPU: argument checks that need no device, the planner-side
method against both header sets, and the C++ program of tests/cpp/path_jobs_interface_test.cpp
(test_path_jobs_interface below runs it on the GPU)."""
import os
import subprocess
import tempfile

import pytest

from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd.build import MOCK_WORKSPACE, ROOT

INCLUDE = os.path.join(ROOT, "include")


def test_path_jobs_entries_refuse_a_null_context(fks_lib):
    jobs = (_capi.PathJob * 1)()
    jobs[0].num_legs = 1
    assert fks_lib.fks_forward_simulate_path_jobs(None, jobs, 1) == 1
    assert fks_lib.fks_forward_simulate_path_jobs_device(None, jobs, 1, None, 1) == 1
    assert fks_lib.fks_multi_forward_simulate_path_jobs(None, jobs, 1) == 1


# the drop-in class of a planner (any robot family) and the plain class over flat configurations
DROP_IN = """
#include "fast_kinematic_simulator_amd/fast_kinematic_simulator.hpp"
namespace upc = uncertainty_planning_core;
typedef tnuva_robot_models::TnuvaSE3Robot<upc::PRNG> Robot;
typedef simple_particle_contact_simulator::HipParticleContactSimulator<Robot, upc::SE3Config, upc::PRNG, upc::SE3ConfigAlloc> Hip;
typedef simple_simulator_interface::SimulatorInterface<upc::SE3Config, upc::PRNG, upc::SE3ConfigAlloc> Interface;
size_t edges(Hip& sim, const std::shared_ptr<Interface::BaseRobotType>& robot,
             const std::vector<upc::SE3Config, upc::SE3ConfigAlloc>& starts, const std::vector<upc::SE3Config, upc::SE3ConfigAlloc>& targets) {
    std::vector<Hip::SimulationPathJob> batch(2);
    batch[0].start_positions = starts;
    batch[0].waypoints = {targets, starts}; /* forward to the targets and back */
    batch[0].allow_contacts = true;
    batch[1] = batch[0];
    batch[1].waypoints.pop_back(); /* a forward-only edge beside it */
    const std::vector<std::vector<std::vector<Interface::SimulationResult>>> results = sim.ForwardSimulateRobotsJobsAlongPaths(robot, batch);
    return results.empty() ? 0 : results.front().back().size();
}
typedef tnuva_robot_models::TnuvaLinkedRobot<upc::PRNG> Arm;
typedef simple_particle_contact_simulator::HipParticleContactSimulator<Arm, upc::LinkedConfig, upc::PRNG, upc::LinkedConfigAlloc> HipArm;
bool edges_arm(HipArm& sim, const std::shared_ptr<HipArm::BaseRobotType>& robot, const std::vector<HipArm::SimulationPathJob>& batch) {
    return sim.ForwardSimulateRobotsJobsAlongPaths(robot, batch).front().front().front().did_contact;
}
int main() { return 0; }
"""

PLAIN = """
#include "fast_kinematic_simulator_amd/hip_particle_contact_simulator.hpp"
uint32_t edges(fks::HipParticleContactSimulator& sim, const fks::RobotDescription& robot, const std::vector<fks::Configuration>& starts,
               const std::vector<fks::Configuration>& targets) {
    const std::vector<fks::SimulationPathJob> batch = {{starts, {targets, starts}, true}, {starts, {targets}, false}};
    const std::vector<std::vector<std::vector<fks::SimulationResult>>> results = sim.ForwardSimulateRobotsJobsAlongPaths(robot, batch);
    return results.front().back().front().microsteps;
}
int main() { return 0; }
"""


@pytest.mark.parametrize("workspace", [False, True], ids=["standalone", "workspace"])
@pytest.mark.parametrize("snippet", [DROP_IN, PLAIN], ids=["drop_in", "plain"])
def test_path_jobs_method_compiles_against_both_header_sets(snippet, workspace):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.cpp")
        with open(path, "w") as f:
            f.write(snippet)
        cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only"] + ([f"-I{MOCK_WORKSPACE}"] if workspace else []) + [f"-I{INCLUDE}", path]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]


def test_path_jobs_program_builds_and_reports_a_missing_device():
    """g++ over the public headers; without a GPU the factory reports FKS_ERR_NO_DEVICE (exit 3)
    after the scene was built, as the planner program does."""
    from fast_kinematic_simulator_amd.build import build_path_jobs_test

    exe = build_path_jobs_test()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode in (0, 3), (p.stdout, p.stderr)
    if p.returncode == 3:
        assert "no HIP device" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("devices,shard", [(None, None), ("0,0", 1)], ids=["one_device", "sharded_0_0"])
def test_path_jobs_interface(fks_lib, devices, shard):
    """ForwardSimulateRobotsJobsAlongPaths equals the sequence of ForwardSimulateRobotsAlongPath
    calls of a second simulator bit for bit (the program compares and exits non-zero on any
    difference), on one device and sharded over two contexts of device 0."""
    from fast_kinematic_simulator_amd.build import build_path_jobs_test

    exe = build_path_jobs_test()
    env = dict(os.environ)
    env.pop("FKS_TEST_DEVICES", None)
    env.pop("FKS_TEST_SHARD", None)
    if devices is not None:
        env["FKS_TEST_DEVICES"] = devices
        env["FKS_TEST_SHARD"] = str(shard)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert " 0 differences" in p.stdout, p.stdout
    want = "devices 2 sharded 1 over 2" if devices else "devices 1 sharded 0 over 1"
    assert p.stderr.count(want) == 1, p.stderr
