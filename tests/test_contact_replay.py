"""The HIP kernels' contact resolution held to the definitions, iteration by iteration.

The replay of tests/test_contact_replay_cpu.py on traces the traced kernels wrote (call index 0, the
same scenes, bounds, caps and verdict checks): the traced linked, SE(2) and SE(3) kernels, the lean
traced kernel (cfg5) and the individual-Jacobian solve (fks_set_individual_jacobians).  tests/
test_trace.py and the parity tests hold the untraced, shaped, small-batch and segmented kernels
bit-equal to the traced results, so they inherit the check.  CheckConfigCollision is compared on 256
configurations of cfg3, of `mixed_tree` and of the telescope at inflation 0 and 0.5, at least 10 % of
which change their verdict between the two ratios."""
import numpy as np
import pytest

import contact_replay as R


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_gpu_iterations_match_reference(fks_lib, name):
    from fast_kinematic_simulator_amd import make_linked_simulator

    wl, individual = R.scene(name, device=0)
    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    try:
        sim.set_individual_jacobians(individual)
        sim.set_call_index(0)
        g, buf = sim.forward_simulate_traced(wl.robot, wl.starts, wl.targets, True, config_capacity=R.CONFIG_CAPACITY)
    finally:
        sim.close()
    assert not np.any(g["error_flags"]), np.unique(g["error_flags"])
    stats = R.replay_scene(name, wl, buf, individual)
    assert stats["compared"] > 0
    if name in ("folding_arm", "telescope", "resolver_params"):
        assert stats["self_corrected"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.CHECK_SCENES)
def test_gpu_config_checks_match_reference(fks_lib, name):
    from fast_kinematic_simulator_amd import make_linked_simulator

    wl, configs = R.check_workload(name)
    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    try:
        results = [sim.check_config_collisions(wl.robot, configs, inflation) for inflation in R.CHECK_INFLATIONS]
    finally:
        sim.close()
    assert not any(np.any(g["error_flags"]) for g in results)
    R.compare_config_checks(name, [g["collided"] for g in results])
