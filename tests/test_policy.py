"""Policy roll-outs in one launch (fks_forward_simulate_policy, the *_policy kernels).

The contract: the call at call index c returns, byte for byte, what the sequence of
include/fks_capi.h returns: before every leg each active particle selects its entry with
fks_policy_select, lost and arrived particles stop, the others run one plain call per contiguous
run of active particles (first_particle_id = the run's first particle, call index c + k) towards
their entries' targets.  The reference in every case is that sequence on a second simulator with
the same seed (tests/policy_cases.py: reference_chain); every comparison is exact and covers
every byte of all eight outputs, the statistics, the work counters, calls == 1 and the final call
index.  Each case first asserts, on the reference's side, the properties that keep it from
passing vacuously.  out_choice and out_distance are fks_policy_select's by construction of the
reference, row K included; every case also asserts it on the call's own outputs: the twin."""
import numpy as np
import pytest

import policy_cases as PC
from fast_kinematic_simulator_amd import PolicyTable, _capi, policy_select
from fast_kinematic_simulator_amd import workloads as W

pytestmark = pytest.mark.gpu

BASE_CALL = 5
OUTPUTS = PC.FIELDS + ("choice", "distance", "legs_run")
WORK = ("particles", "controller_steps", "microsteps", "resolver_iterations", "sdf_bytes", "error_particles", "least_squares_rows",
        "self_collision_checks", "self_corrected_points")


def _sim(wl, segment_steps=None, small_batch=None):
    from fast_kinematic_simulator_amd import make_linked_simulator

    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    sim.set_specialization(False)
    if segment_steps is not None:
        sim.set_segment_steps(segment_steps)
    if small_batch is not None:
        sim.set_small_batch_kernel(small_batch)
    return sim


def _reference(wl, starts, table, K, allow=True, call=BASE_CALL):
    """reference_chain over forward_simulate_device on a second simulator"""
    import torch

    dev = torch.device("cuda", 0)
    sim = _sim(wl)
    counters = dict.fromkeys(WORK, 0)
    Wd = wl.robot.config_width
    try:
        def simulate(k, a, q, targets):
            m = q.shape[0]
            d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
            d_t = torch.from_numpy(np.ascontiguousarray(targets)).to(dev)
            out = torch.empty((m, Wd), dtype=torch.float64, device=dev)
            coll = torch.empty(m, dtype=torch.uint8, device=dev)
            micro, res, err = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(3))
            sim.set_call_index(call + k)
            sim.forward_simulate_device(wl.robot, d_q.data_ptr(), m, d_t.data_ptr(), m, a, allow, out.data_ptr(), coll.data_ptr(),
                                        micro.data_ptr(), res.data_ptr(), err.data_ptr(), synchronize=True)
            c = sim.last_call_counters()
            for key in WORK:
                counters[key] += c[key]
            return {"positions": out.cpu().numpy(), "collided": coll.cpu().numpy().astype(bool),
                    "microsteps": micro.cpu().numpy().astype(np.uint32), "resolver_iterations": res.cpu().numpy().astype(np.uint32),
                    "error_flags": err.cpu().numpy().astype(np.uint32)}

        ref = PC.reference_chain(simulate, wl.robot, starts, table, K)
        assert counters["particles"] == ref["pairs"]
        ref["statistics"] = sim.get_statistics()
        ref["counters"] = counters
        return ref
    finally:
        sim.close()


def _policy(wl, starts, table, K, allow=True, call=BASE_CALL, **settings):
    sim = _sim(wl, **settings)
    try:
        sim.set_call_index(call)
        r = sim.forward_simulate_policy_arrays(wl.robot, starts, table, K, allow)
        r["statistics"] = sim.get_statistics()
        r["counters"] = sim.last_call_counters()
        r["call_index"] = sim.get_call_index()
        r["launch"] = sim.launch_info()
        r["inputs"] = (wl.robot, np.asarray(starts, dtype=np.float64), table)
        return r
    finally:
        sim.close()


def _assert_twin(p, K):
    """every selection of the call, row K included, is fks_policy_select of the configuration
    handed over (the starts, then the row before's positions), bit for bit; the rows after a
    particle's stop are NONE and +inf"""
    robot, starts, table = p["inputs"]
    for k in range(K + 1):
        ran = p["legs_run"] >= k
        q = starts if k == 0 else p["positions"][k - 1]
        sel = policy_select(robot, table, q[ran])
        assert np.array_equal(p["choice"][k][ran], sel["choice"]), k
        assert np.array_equal(p["distance"][k][ran], sel["distance"]), k
        assert np.all(p["choice"][k][~ran] == _capi.POLICY_NONE) and np.all(p["distance"][k][~ran] == np.inf)


def _assert_is_reference(p, ref, K, call=BASE_CALL):
    _assert_twin(p, K)
    for f in OUTPUTS:
        assert p[f].shape == ref[f].shape and p[f].dtype == ref[f].dtype, f
        assert np.array_equal(p[f], ref[f]), (f, np.argwhere(p[f] != ref[f])[:8].tolist())
    assert p["statistics"] == ref["statistics"]
    for key in WORK:
        assert p["counters"][key] == ref["counters"][key], (key, p["counters"][key], ref["counters"][key])
    assert p["counters"]["calls"] == 1
    assert p["call_index"] == call + K


# ---- 1: SE(2), cfg1, 32 particles, K = 6, M = 70
@pytest.fixture(scope="module")
def cfg1_refs(fks_lib):
    out = {}
    for max_distance in (1.2, np.inf):
        wl, starts, table, K = PC.cfg1_case(max_distance)
        out[max_distance] = _reference(wl, starts, table, K)
        PC.check_cfg1(out[max_distance], K)
    return out


@pytest.mark.parametrize("max_distance", [1.2, np.inf], ids=["max_1.2", "max_inf"])
def test_se2_small_batch_policy(fks_lib, cfg1_refs, max_distance):
    wl, starts, table, K = PC.cfg1_case(max_distance)
    p = _policy(wl, starts, table, K)
    assert p["launch"]["last_kernel"] == "policy_small_batch"
    _assert_is_reference(p, cfg1_refs[max_distance], K)
    if max_distance == 1.2:
        assert (p["choice"] == _capi.POLICY_LOST).any()


@pytest.mark.parametrize("max_distance", [1.2, np.inf], ids=["max_1.2", "max_inf"])
def test_se2_segmented_policy_runs_the_throughput_kernel(fks_lib, cfg1_refs, max_distance):
    """50 steps in segments of 7: a partial last segment in every leg, a later segment's wave reads
    the leg's choice back, and a stopped particle's later tickets are stale"""
    wl, starts, table, K = PC.cfg1_case(max_distance)
    p = _policy(wl, starts, table, K, segment_steps=7)
    assert p["launch"]["last_kernel"] == "policy"
    _assert_is_reference(p, cfg1_refs[max_distance], K)


@pytest.mark.parametrize("max_distance", [1.2, np.inf], ids=["max_1.2", "max_inf"])
def test_se2_whole_policy_on_the_throughput_kernel(fks_lib, cfg1_refs, max_distance):
    wl, starts, table, K = PC.cfg1_case(max_distance)
    p = _policy(wl, starts, table, K, small_batch=False)
    assert p["launch"]["last_kernel"] == "policy"
    _assert_is_reference(p, cfg1_refs[max_distance], K)


# ---- 2: more particles than resident waves
def test_more_particles_than_resident_waves(fks_lib):
    """automatic segments, ticket claims, and particles that stop at leg 0 or 1 while their
    neighbours run on"""
    wl, starts, table, _ = PC.cfg1_case(np.inf)
    sim = _sim(wl)
    try:
        sim.set_robot(wl.robot)
        n = sim.launch_info()["resident_waves"] + 1000
    finally:
        sim.close()
    starts = np.tile(starts, (n // len(starts) + 1, 1))[:n]
    K = 2
    ref = _reference(wl, starts, table, K)
    hist = np.bincount(ref["legs_run"], minlength=K + 1)
    assert hist[0] > 0 and hist[1] > 0 and hist[2] > n // 2, hist
    assert ref["collided"].any(axis=1).all()
    p = _policy(wl, starts, table, K)
    assert p["launch"]["last_kernel"] == "policy"
    _assert_is_reference(p, ref, K)


# ---- 3: linked robots
@pytest.mark.parametrize("segment_steps", [None, 9], ids=["whole", "segments_of_9"])
def test_linked_continuous_self_contact_policy(fks_lib, segment_steps):
    wl, starts, table, K = PC.folding_case()
    ref = _reference(wl, starts, table, K)
    PC.check_arm(ref, K)
    assert ref["counters"]["self_collision_checks"] > 0
    p = _policy(wl, starts, table, K, segment_steps=segment_steps)
    whole_kernel = "policy" if p["launch"]["lean"] else "policy_small_batch"  # no small-batch kernel for a lean block
    assert p["launch"]["last_kernel"] == ("policy" if segment_steps else whole_kernel)
    _assert_is_reference(p, ref, K)


@pytest.fixture(scope="module")
def cfg3_ref(fks_lib):
    wl, starts, table, K = PC.cfg3_case()
    ref = _reference(wl, starts, table, K)
    PC.check_arm(ref, K)
    return ref


@pytest.mark.parametrize("segment_steps", [None, 9], ids=["whole", "segments_of_9"])
def test_linked_7dof_policy(fks_lib, cfg3_ref, segment_steps):
    wl, starts, table, K = PC.cfg3_case()
    p = _policy(wl, starts, table, K, segment_steps=segment_steps)
    assert p["launch"]["last_kernel"] == ("policy" if segment_steps else "policy_small_batch")
    _assert_is_reference(p, cfg3_ref, K)


# ---- 4: SE(3)
def test_se3_policy(fks_lib):
    wl, starts, table, K = PC.cfg4_case()
    ref = _reference(wl, starts, table, K)
    PC.check_cfg4(ref, K)
    p = _policy(wl, starts, table, K)
    assert p["launch"]["last_kernel"] == "policy_small_batch"
    _assert_is_reference(p, ref, K)


# ---- 5: the twin, stated on the call's own outputs: _assert_twin, in every case above and
# below (each _assert_is_reference begins with it), and here on its own so that it is named
def test_choices_and_distances_are_the_host_twins(fks_lib):
    wl, starts, table, K = PC.cfg1_case(1.2)
    p = _policy(wl, starts, table, K)
    assert (p["legs_run"] < K).any() and (p["legs_run"] == K).any()  # rows after a stop, and row K
    _assert_twin(p, K)


# ---- 6: shards through the device entry
def test_shards_equal_the_whole_call(fks_lib, cfg1_refs):
    import torch

    dev = torch.device("cuda", 0)
    wl, starts, table, K = PC.cfg1_case(1.2)
    ref = cfg1_refs[1.2]
    d_keys = torch.from_numpy(np.ascontiguousarray(table.keys)).to(dev)
    d_targets = torch.from_numpy(np.ascontiguousarray(table.targets)).to(dev)
    d_flags = torch.from_numpy(np.where(table.terminal, 1, 0).astype(np.int32)).to(dev)
    sim = _sim(wl)
    try:
        for a, b in ((0, 11), (11, 32)):
            m = b - a
            d_q = torch.from_numpy(np.ascontiguousarray(starts[a:b])).to(dev)
            out = torch.empty((K, m, 3), dtype=torch.float64, device=dev)
            coll = torch.empty((K, m), dtype=torch.uint8, device=dev)
            micro, res, err = (torch.empty((K, m), dtype=torch.int32, device=dev) for _ in range(3))
            choice = torch.empty((K + 1, m), dtype=torch.int32, device=dev)
            dist = torch.empty((K + 1, m), dtype=torch.float64, device=dev)
            legs = torch.empty(m, dtype=torch.int32, device=dev)
            sim.set_call_index(BASE_CALL)
            sim.forward_simulate_policy_device(wl.robot, d_q.data_ptr(), m, d_keys.data_ptr(), d_targets.data_ptr(), d_flags.data_ptr(),
                                               70, table.terminal_distance, table.max_distance, K, a, True, out.data_ptr(),
                                               choice.data_ptr(), dist.data_ptr(), legs.data_ptr(), coll.data_ptr(), micro.data_ptr(),
                                               res.data_ptr(), err.data_ptr(), synchronize=True)
            assert sim.get_call_index() == BASE_CALL + K
            got = {"positions": out.cpu().numpy(), "collided": coll.cpu().numpy().astype(bool),
                   "microsteps": micro.cpu().numpy().astype(np.uint32), "resolver_iterations": res.cpu().numpy().astype(np.uint32),
                   "error_flags": err.cpu().numpy().astype(np.uint32), "choice": choice.cpu().numpy().astype(np.uint32),
                   "distance": dist.cpu().numpy(), "legs_run": legs.cpu().numpy().astype(np.uint32)}
            for f in OUTPUTS:
                want = ref[f][a:b] if f == "legs_run" else ref[f][:, a:b]
                assert np.array_equal(got[f], want), (a, b, f)
    finally:
        sim.close()


# ---- 7: degenerate
def test_one_leg_and_one_entry(fks_lib):
    wl, starts, table, _ = PC.cfg1_case(1.2)
    ref = _reference(wl, starts, table, 1)
    assert (ref["legs_run"] == 0).any() and (ref["legs_run"] == 1).any()
    _assert_is_reference(_policy(wl, starts, table, 1), ref, 1)
    one = PolicyTable(table.keys[3:4], table.targets[3:4], np.array([True]), terminal_distance=0.3, max_distance=np.inf)
    ref = _reference(wl, starts, one, 3)
    assert np.all((ref["choice"][ref["choice"] < _capi.POLICY_LOST] & PC.INDEX) == 0)
    _assert_is_reference(_policy(wl, starts, one, 3), ref, 3)


def test_without_a_terminal_entry_it_is_a_path_over_the_chosen_waypoints(fks_lib):
    wl, starts, table, K = PC.cfg1_case(np.inf)
    table = PolicyTable(table.keys, table.targets, None, 0.0, np.inf)
    ref = _reference(wl, starts, table, K)
    assert np.all(ref["legs_run"] == K)
    p = _policy(wl, starts, table, K)
    _assert_is_reference(p, ref, K)
    waypoints = np.asarray(table.targets)[ref["choice"][:K] & PC.INDEX]  # [K][n][W]: what each particle chose
    sim = _sim(wl)
    try:
        sim.set_call_index(BASE_CALL)
        path = sim.forward_simulate_path_arrays(wl.robot, starts, waypoints, True)
        for f in PC.FIELDS:
            assert np.array_equal(path[f], p[f]), f
        assert sim.get_statistics() == p["statistics"]
    finally:
        sim.close()


def test_no_particles_consume_the_call_indices_and_refusals_none(fks_lib):
    wl, starts, table, K = PC.cfg1_case(1.2)
    sim = _sim(wl)
    try:
        sim.set_call_index(BASE_CALL)
        r = sim.forward_simulate_policy_arrays(wl.robot, np.zeros((0, 3)), table, K, True)
        assert r["positions"].shape == (K, 0, 3) and r["choice"].shape == (K + 1, 0)
        assert sim.get_call_index() == BASE_CALL + K
        sim.set_call_index(BASE_CALL)
        nan = float("nan")
        refused = [
            (PolicyTable(table.keys, table.targets, table.terminal, 0.6, 1.2), 0, "at least one leg"),
            (PolicyTable(table.keys, table.targets, table.terminal, nan, 1.2), K, "NaN"),
            (PolicyTable(table.keys, table.targets, table.terminal, 0.6, nan), K, "NaN"),
            (PolicyTable(np.zeros((0, 3)), np.zeros((0, 3)), None, 0.6, 1.2), K, "at least one entry"),
        ]
        for bad, legs, text in refused:
            with pytest.raises(_capi.FksError) as e:
                sim.forward_simulate_policy_arrays(wl.robot, starts, bad, legs, True)
            assert e.value.status == 1 and text in str(e.value), str(e.value)
            assert sim.get_call_index() == BASE_CALL
        # The device entry's refusals come before any pointer is read; the table's and the legs' hold
        # for n == 0 too, so these calls name no buffer at all (8 stands for a table array in HBM).
        # legs x segments per leg >= 2^31 (50 steps in segments of 1)
        sim.set_segment_steps(1)
        with pytest.raises(_capi.FksError) as e:
            sim.forward_simulate_policy_device(wl.robot, 0, 0, 8, 8, 0, 70, 0.6, 1.2, 2 ** 31 // 50 + 1, 0, True, 0, 0)
        assert e.value.status == 1 and "2^31" in str(e.value)
        with pytest.raises(_capi.FksError) as e:
            sim.forward_simulate_policy_device(wl.robot, 0, 0, 8, 8, 0, 2 ** 30 + 1, 0.6, 1.2, K, 0, True, 0, 0)
        assert e.value.status == 1 and "2^30" in str(e.value)
        with pytest.raises(_capi.FksError) as e:
            sim.forward_simulate_policy_device(wl.robot, 0, 0, 0, 8, 0, 70, 0.6, 1.2, K, 0, True, 0, 0)
        assert e.value.status == 1 and "keys or targets" in str(e.value)
        # a null out_choice with n > 0 (the host entry: nothing has been staged yet)
        ctable, keep = table.to_c(3)
        q = np.ascontiguousarray(starts)
        out = np.zeros((K, len(q), 3))
        st = fks_lib.fks_forward_simulate_policy(sim._ctx, _capi.as_ptr(q, _capi.c_double), len(q), ctable, K, 1,
                                                 _capi.as_ptr(out, _capi.c_double), None, None, None, None, None, None, None)
        assert st == 1 and b"null host buffer" in fks_lib.fks_get_last_error(sim._ctx)
        assert sim.get_call_index() == BASE_CALL
        sim.set_segment_steps(0)
        sim.set_individual_jacobians(True)
        with pytest.raises(_capi.FksError) as e:
            sim.forward_simulate_policy_arrays(wl.robot, starts, table, K, True)
        assert e.value.status == 5 and "individual Jacobians" in str(e.value)
        assert sim.get_call_index() == BASE_CALL
    finally:
        sim.close()
