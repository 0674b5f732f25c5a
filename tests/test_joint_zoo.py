"""The HIP path on the joint zoo (tests/joint_zoo.py): prismatic and continuous joints, oblique and
non-unit axes, rotated origins, a branched tree, a 10-dof chain.

Kinematics: bit for bit against the oracle and, directly, against the high-precision reference
with the tolerances of tests/test_joint_zoo_cpu.py.  Simulation: every output, counter and
statistic bit for bit against the oracle on every kernel family, with the scenes' non-vacuity
conditions asserted on the GPU result; traces; the configuration check; one path-jobs batch.
Skip proofs: the shaped kernel against the same kernel with every proof compiled out, at 512
particles -- the test a wrong prismatic lever arm (fks_set_robot) fails."""
import functools

import numpy as np
import pytest

import joint_zoo as Z
from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd import make_linked_simulator

from parity_util import COUNTER_KEYS, assert_counters_identical, assert_identical, mismatch_report, run_both
from test_joint_zoo_cpu import check_apply_control_input, control_cases, kinematics_ratios, xform, zoo_configs

pytestmark = pytest.mark.gpu

KEYS = ("positions", "collided", "microsteps", "resolver_iterations", "error_flags")


@functools.lru_cache(maxsize=None)
def scene(name, n=16):
    return Z.SCENES[name](n)


def _simulator(wl):
    return make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)


# ---------------------------------------------------------------- kinematics
@pytest.mark.parametrize("name", Z.MEASURABLE)
def test_kinematics_match_oracle_and_reference(fks_lib, oracle_lib, name):
    import oracle

    wl = scene(name)
    robot = wl.robot
    cfgs = zoo_configs(robot)
    q, u, vmax = control_cases(robot)
    sim = _simulator(wl)
    try:
        T = sim.link_transforms(robot, cfgs)
        P = sim.world_points(robot, cfgs)
        A = sim.apply_control_input(robot, q, u)
    finally:
        sim.close()
    pts = robot.geometry_points
    worst_t = worst_p = 0.0
    for i, c in enumerate(cfgs):
        To = oracle.link_transforms(robot, c)  # per geometry
        mine = [T[i, robot.geometry_link[g]].reshape(12) for g in range(len(pts))]
        for g in range(len(pts)):
            assert np.array_equal(mine[g], To[g]), (i, g)
        assert np.array_equal(P[i], np.concatenate([xform(To[g], np.asarray(pts[g])) for g in range(len(pts))], axis=0)), i
        rt, rp = kinematics_ratios(robot, c, mine, P[i])
        worst_t, worst_p = max(worst_t, rt), max(worst_p, rp)
    print(f"{name} (GPU): worst ratio to the bound: link transforms {worst_t:.3f}, world points {worst_p:.3f}")
    assert worst_t <= 1.0 and worst_p <= 1.0
    for i in range(len(q)):
        assert np.array_equal(A[i], oracle.apply_control_input(robot, q[i], u[i])), i
    check_apply_control_input(robot, q, u, vmax, A, name + " (GPU)")


# ---------------------------------------------------------------- simulation parity
EVERY_SCENE = {"default": {}, "throughput": {"small_batch_kernel": False}, "segments_of_3": {"segment_steps": 3}}
MORE = {"individual_jacobians": {"individual_jacobians": True}, "specialize": {"specialize": True},
        "cooperative": {"cooperative": 1, "small_batch_kernel": True}, "no_contacts": {"allow_contacts": False}}
PARITY = [(name, v) for name in Z.SCENES for v in EVERY_SCENE] + [(name, v) for name in ("mixed_tree", "gantry") for v in MORE]


@pytest.mark.parametrize("name,variant", PARITY)
def test_simulation_parity(fks_lib, oracle_lib, name, variant):
    wl = scene(name)
    g, o = run_both(wl, call_index=4, **{**EVERY_SCENE, **MORE}[variant])
    print(name, variant, g["launch"]["last_kernel"], mismatch_report(g, o), g["counters"])
    assert_identical(g, o)
    assert_counters_identical(g, o)
    if variant == "throughput":
        assert g["launch"]["last_kernel"] == "throughput", g["launch"]
    if variant == "cooperative":
        assert g["launch"]["last_kernel"] == "cooperative", g["launch"]
    if variant == "no_contacts":
        # a contact ends the particle's simulation and leaves its flag clear (SPCS:1776-1779, 904-909)
        assert not g["collided"].any() and not g["error_flags"].any()
        assert 0 < g["counters"]["controller_steps"] < wl.num_particles * wl.steps
    else:
        Z.check_scene(name, wl, g)


# ---------------------------------------------------------------- trace
@pytest.mark.parametrize("name", ["mixed_tree", "gantry"])
def test_trace_matches_oracle(fks_lib, oracle_lib, name):
    import oracle

    wl = scene(name, 8)
    sim = _simulator(wl)
    try:
        sim.set_call_index(0)
        g, gb = sim.forward_simulate_traced(wl.robot, wl.starts, wl.targets, True, config_capacity=8192)
    finally:
        sim.close()
    o, ob = oracle.forward_simulate_traced(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, wl.starts,
                                           wl.targets, True, config_capacity=8192)
    assert int(np.max(ob.num_configs)) <= ob.config_capacity and o["resolver_iterations"].sum() > 0
    for k in KEYS:
        assert np.array_equal(g[k], o[k]), k
    for k in ("num_steps", "num_configs", "step_microsteps", "step_inputs", "config_tags", "configs"):
        assert np.array_equal(getattr(gb, k), getattr(ob, k)), k


# ---------------------------------------------------------------- skip proofs
def _run(sim, wl, mode, call_index):
    sim.set_specialization(mode)
    info = sim.specialization()
    assert info["active"] and not info["failed"], info
    assert info["shape"].endswith("-np") == (mode == _capi.SPECIALIZE_NO_PROOFS), info
    sim.set_call_index(call_index)
    sim.reset_statistics()
    r = sim.forward_simulate_arrays(wl.robot, wl.starts, wl.targets, wl.allow_contacts)
    assert sim.launch_info()["last_kernel"] == "shaped", sim.launch_info()
    r["counters"] = sim.last_call_counters()
    r["statistics"] = sim.get_statistics()
    return r


@pytest.mark.parametrize("name", ["mixed_tree", "gantry", "telescope", "skew_axis"])
def test_skip_proofs_change_nothing(fks_lib, oracle_lib, name):
    """The lever arms of the skip proofs (fks_set_robot: |axis| for a prismatic dof, the largest
    stroke added to the reach of the revolute dofs upstream, no lever for a non-unit revolute axis)
    bound how far a step can move a point.  A lever that is too short skips work that would have
    changed the result: the product kernel then differs from the proof-free one.  skew_axis: the
    non-unit axis stretches whatever hangs behind it, so the finite levers of the dofs around it
    bound nothing; every proof sums over all dofs, the skewed dof's infinite lever among them, so
    none may pass for this robot."""
    import oracle

    wl = scene(name, 512)
    sim = _simulator(wl)
    try:
        sim.set_robot(wl.robot)
        sim.set_small_batch_kernel(False)
        p = _run(sim, wl, _capi.SPECIALIZE_ON, 7)
        q = _run(sim, wl, _capi.SPECIALIZE_NO_PROOFS, 7)
    finally:
        sim.close()
    print(name, "product", p["counters"]["kernel_ms"], "ms; proof-free", q["counters"]["kernel_ms"], "ms;", p["counters"])
    for k in KEYS:
        assert np.array_equal(p[k], q[k]), (k, int(np.sum(np.any(np.atleast_2d(p[k] != q[k]).reshape(512, -1), axis=1))))
    for k in COUNTER_KEYS:
        assert p["counters"][k] == q["counters"][k], (k, p["counters"][k], q["counters"][k])
    assert p["statistics"] == q["statistics"]
    assert p["counters"]["resolver_iterations"] > 0 and p["collided"].any()
    o = oracle.forward_simulate(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, wl.starts[:32], wl.targets,
                                True, call_index=7)
    for k in KEYS:
        assert np.array_equal(q[k][:32], o[k]), k


# ---------------------------------------------------------------- configuration check
def _check_configs(robot, n=256, seed=3):
    lo, hi = robot.dof_limits()
    return np.random.default_rng(seed).uniform(lo, hi, size=(n, robot.config_width))


def _assert_check_parity(sim, wl, cfgs, kernel):
    import oracle

    for inflation in (0.0, 0.5):
        g = sim.check_config_collisions(wl.robot, cfgs, inflation)
        assert sim.launch_info()["last_check_kernel"] == kernel, sim.launch_info()
        o = oracle.check_config_collision(wl.environment(), wl.robot, wl.solver, cfgs, inflation)
        assert np.array_equal(g["collided"], o["collided"]), np.nonzero(g["collided"] != o["collided"])[0][:8]
        assert np.array_equal(g["error_flags"], o["error_flags"])
        assert sim.last_check_counters()["sdf_bytes"] == int(o["sdf_bytes"].sum())
        assert 0 < int(g["collided"].sum()) < len(cfgs)  # both verdicts


@pytest.mark.parametrize("name", ["mixed_tree", "gantry", "telescope"])
def test_config_check_parity(fks_lib, oracle_lib, name):
    wl = scene(name)
    sim = _simulator(wl)
    try:
        sim.set_specialization(False)
        _assert_check_parity(sim, wl, _check_configs(wl.robot), "throughput")
    finally:
        sim.close()


def test_shaped_config_check_parity(fks_lib, oracle_lib):
    """The shape-specialised check comes with the simulation kernel's module: a shaped simulation
    builds it, the checks after it run it."""
    wl = scene("mixed_tree")
    sim = _simulator(wl)
    try:
        sim.set_robot(wl.robot)
        sim.set_small_batch_kernel(False)
        sim.forward_simulate_arrays(wl.robot, wl.starts[:4], wl.targets, True)
        assert sim.launch_info()["last_kernel"] == "shaped", sim.launch_info()
        _assert_check_parity(sim, wl, _check_configs(wl.robot), "shaped")
    finally:
        sim.close()


# ---------------------------------------------------------------- batched entries
def test_path_jobs_equal_path_calls(fks_lib):
    """3 jobs of 2, 1 and 2 legs, 8 particles each, on the generic batched kernels: byte for byte the
    corresponding sequence of path calls (the PATH and JOBS instantiations on the zoo's robot)."""
    from test_path_jobs import _assert_batch_is_sequence, _assert_not_vacuous, _batch, _sequence

    wl = scene("mixed_tree")
    home = Z.MIXED_NOMINAL[None]
    jobs = [(wl.starts[:8], [wl.targets, home], True),
            (wl.starts[8:16], [wl.targets], True),
            (wl.starts[:8], [0.5 * (home + wl.targets), home], False)]
    s = _sequence(wl, jobs)
    _assert_not_vacuous(s, jobs, colliding=(0, 1))
    assert s["jobs"][0]["resolver_iterations"].sum() > 0
    b = _batch(wl, jobs)
    assert b["launch"]["last_kernel"] in ("path_jobs", "path_jobs_small_batch"), b["launch"]
    _assert_batch_is_sequence(b, s, jobs)
