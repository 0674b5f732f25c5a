"""The host entries' staging buffers across growth and reuse (csrc/fks_buffers.h).

One simulator runs every host entry at 2, then 67, then 2, then 131 particles, so that each staging
buffer grows, is reused below its capacity and grows again; the multi-device simulator does the same
for the entries it has.  The contract: what a call returns does not depend on what the context staged
before it.  Every step's arrays and work counters equal, byte for byte, the same call at the same
call index on a simulator created for that call alone.  The fresh side first shows that particles
collided, so the comparison cannot pass on runs in which nothing happened."""
import numpy as np
import pytest

from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd import workloads as W
from fast_kinematic_simulator_amd.simulator import MultiDeviceSimulator, PolicyTable

pytestmark = pytest.mark.gpu

SIZES = (2, 67, 2, 131)
WORK = ("particles", "controller_steps", "microsteps", "resolver_iterations", "sdf_bytes", "error_particles", "least_squares_rows",
        "self_collision_checks", "self_corrected_points")
STEPS = ("simulate", "check", "path", "jobs", "path_jobs", "policy", "mutable", "cluster")
MULTI_STEPS = ("simulate", "check", "path", "jobs", "path_jobs")


def _call_index(round_index, step):
    return 1000 * round_index + 20 * STEPS.index(step) + 3


def _inputs(wl, n):
    """the arguments of every step at n particles: per-particle targets, so the targets grow too"""
    rng = np.random.default_rng(100 + n)
    starts = wl.starts[:n]
    spots = lambda *shape: np.stack([rng.uniform(0.4, 3.6, shape), rng.uniform(0.4, 3.6, shape), rng.uniform(-3, 3, shape)], axis=-1)
    return {"starts": starts, "targets": spots(n), "way": spots(3, n), "one": spots(1), "short_way": spots(2, 1),
            "table": PolicyTable(spots(4), spots(4), np.array([False, False, False, True]), terminal_distance=0.3, max_distance=np.inf)}


def _work(counters):
    return {key: counters[key] for key in WORK}


def _step(sim, wl, step, a, multi=False):
    """one host entry: its arrays (a dict or a list of dicts) and its work counters (None: it has none)"""
    robot, starts = wl.robot, a["starts"]
    if step == "simulate":
        return sim.forward_simulate_arrays(robot, starts, a["targets"], True), _work(sim.last_call_counters())
    if step == "check":
        r = sim.check_config_collisions(robot, a["targets"], 0.5)
        if multi:
            return {"collided": r[0], "error_flags": r[1]}, None
        return r, {key: sim.last_check_counters()[key] for key in ("particles", "sdf_bytes")}
    if step == "path":
        return sim.forward_simulate_path_arrays(robot, starts, a["way"], True), _work(sim.last_call_counters())
    if step == "jobs":
        jobs = [(starts, a["targets"], True), (starts[:1], a["one"], False), (starts[:0], a["one"], True)]
        return sim.forward_simulate_jobs_arrays(robot, jobs), _work(sim.last_call_counters())
    if step == "path_jobs":
        jobs = [(starts, a["way"], True), (starts[:1], a["short_way"], True), (starts[:0], a["short_way"], False)]
        return sim.forward_simulate_path_jobs_arrays(robot, jobs), _work(sim.last_call_counters())
    if step == "policy":
        return sim.forward_simulate_policy_arrays(robot, starts, a["table"], 2, True), _work(sim.last_call_counters())
    if step == "mutable":
        state = np.zeros((len(starts), 2 * robot.num_dofs))
        r = sim.forward_simulate_mutable_arrays(robot, starts, a["targets"], True, state)
        return dict(r, controller_state=state), _work(sim.last_call_counters())
    assert step == "cluster"
    r = sim.cluster_outcomes(robot, [a["targets"], a["way"][0][: max(1, len(starts) // 2)], a["one"]], 0.8, distances=True)
    return {"counts": r["counts"], **{f"labels{g}": v for g, v in enumerate(r["labels"])},
            **{f"distances{g}": v for g, v in enumerate(r["distances"])}}, None


def _single(wl):
    from fast_kinematic_simulator_amd import make_linked_simulator

    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    sim.set_specialization(False)
    return sim


def _assert_same(got, ref, where):
    if isinstance(ref, list):
        assert len(got) == len(ref), where
        for j, (g, r) in enumerate(zip(got, ref)):
            _assert_same(g, r, where + (j,))
        return
    assert got.keys() == ref.keys(), where
    for key in ref:
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes(), where + (key,)


@pytest.fixture(scope="module")
def case(fks_lib):
    wl = W.cfg1(max(SIZES) / 32.0)
    assert wl.num_particles == max(SIZES)
    return wl, {n: _inputs(wl, n) for n in set(SIZES)}


@pytest.fixture(scope="module")
def fresh(case):
    """every (round, step) on a simulator created for it alone"""
    wl, inputs = case
    out, collided = {}, 0
    for i, n in enumerate(SIZES):
        for step in STEPS:
            sim = _single(wl)
            try:
                sim.set_call_index(_call_index(i, step))
                out[i, step] = _step(sim, wl, step, inputs[n])
            finally:
                sim.close()
        collided += int(out[i, "simulate"][0]["collided"].sum())
        assert out[i, "simulate"][0]["positions"].shape == (n, 3)
    print("contact-allowed particles that collided on the fresh side:", collided)
    assert collided >= 1
    # the call index is part of the result: the two rounds of 2 particles differ
    assert not np.array_equal(out[0, "simulate"][0]["positions"], out[2, "simulate"][0]["positions"])
    return out


def test_one_context_through_growth_and_reuse(case, fresh):
    wl, inputs = case
    sim = _single(wl)
    try:
        for i, n in enumerate(SIZES):
            for step in STEPS:
                sim.set_call_index(_call_index(i, step))
                got, work = _step(sim, wl, step, inputs[n])
                _assert_same(got, fresh[i, step][0], (i, n, step))
                assert work == fresh[i, step][1], (i, n, step)
    finally:
        sim.close()


def test_multi_device_context_through_growth_and_reuse(case, fresh):
    wl, inputs = case
    lib = _capi.lib()
    m = MultiDeviceSimulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed, list(range(lib.fks_device_count())))
    try:
        for shard in range(m.num_devices()):
            ctx = lib.fks_multi_device_context(m._ctx, shard)
            _capi.check(lib.fks_set_specialization(ctx, 0), ctx, "specialization")
        for i, n in enumerate(SIZES):
            for step in MULTI_STEPS:
                m.set_call_index(_call_index(i, step))
                got, work = _step(m, wl, step, inputs[n], multi=True)
                _assert_same(got, fresh[i, step][0], (i, n, step))
                if work is not None:  # the sharded check keeps no counters
                    assert work == fresh[i, step][1], (i, n, step)
    finally:
        m.close()
