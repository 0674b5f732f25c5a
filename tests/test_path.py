"""Waypoint paths in one launch (fks_forward_simulate_path, the *_path kernels).

The contract: path(starts, waypoints[K]) at call index c returns, byte for byte, what K chained
plain calls return (leg k at call index c + k from leg k-1's positions), its statistics and
work counters are the chain's sums, and the call index ends at c + K.  The reference in every
case is that chain on a second simulator with the same seed; every comparison is exact.  Each
case first asserts, on the chain's side, that its legs make contact or end early, so it cannot
pass on legs in which nothing happened."""
import numpy as np
import pytest

from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd import workloads as W

pytestmark = pytest.mark.gpu

BASE_CALL = 5
FIELDS = ("positions", "collided", "microsteps", "resolver_iterations", "error_flags")
# what a call counts of its own work (not its times, and `calls`, which a path counts once)
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


def _chain(wl, starts, legs, allow, call=BASE_CALL, **settings):
    """K chained forward_simulate_arrays calls: per-leg results, statistics and summed work counters."""
    sim = _sim(wl, **settings)
    try:
        q = np.asarray(starts, dtype=np.float64)
        out, counters, per_leg = [], dict.fromkeys(WORK, 0), []
        for k, targets in enumerate(legs):
            sim.set_call_index(call + k)
            r = sim.forward_simulate_arrays(wl.robot, q, targets, allow)
            c = sim.last_call_counters()
            per_leg.append(dict(c, statistics=sim.get_statistics()))
            for key in WORK:
                counters[key] += c[key]
            out.append(r)
            q = r["positions"]
        return {"legs": out, "statistics": sim.get_statistics(), "counters": counters, "per_leg": per_leg,
                "call_index": sim.get_call_index()}
    finally:
        sim.close()


def _path(wl, starts, legs, allow, call=BASE_CALL, sim=None, **settings):
    own = sim is None
    if own:
        sim = _sim(wl, **settings)
    try:
        sim.set_call_index(call)
        r = sim.forward_simulate_path_arrays(wl.robot, starts, np.stack([np.asarray(t, dtype=np.float64) for t in legs]), allow)
        r["statistics"] = sim.get_statistics()
        r["counters"] = sim.last_call_counters()
        r["call_index"] = sim.get_call_index()
        r["launch"] = sim.launch_info()
        return r
    finally:
        if own:
            sim.close()


def _assert_path_is_chain(p, c):
    K = len(c["legs"])
    assert p["positions"].shape[0] == K
    for k in range(K):
        for f in FIELDS:
            assert np.array_equal(p[f][k], c["legs"][k][f]), (k, f)
    assert p["statistics"] == c["statistics"]
    for key in WORK:
        assert p["counters"][key] == c["counters"][key], (key, p["counters"][key], c["counters"][key])
    assert p["counters"]["calls"] == 1
    assert p["call_index"] == c["call_index"] == BASE_CALL + K


def _unsuccessful(c, k):
    """unsuccessful resolves of leg k alone (the statistics accumulate over the chain)"""
    now = c["per_leg"][k]["statistics"]["unsuccessful_resolves"]
    return now - (c["per_leg"][k - 1]["statistics"]["unsuccessful_resolves"] if k else 0)


# ---- 1, 3: SE(2), the small-batch path kernel, and the same path in segments on the throughput kernel
def _cfg1_case():
    wl = W.cfg1(1.0)
    return wl, [wl.targets, [[0.6, 3.4, -1.0]], [[3.4, 0.6, 2.0]]]


@pytest.fixture(scope="module")
def cfg1_chains(fks_lib):
    wl, legs = _cfg1_case()
    return {allow: _chain(wl, wl.starts, legs, allow) for allow in (True, False)}


@pytest.mark.parametrize("allow", [True, False], ids=["contacts", "no_contacts"])
def test_se2_small_batch_path(fks_lib, oracle_lib, cfg1_chains, allow):
    import oracle

    wl, legs = _cfg1_case()
    c = cfg1_chains[allow]
    for k in range(3):
        assert c["per_leg"][k]["controller_steps"] < 32 * 50  # some particles end the leg early
        if allow:
            assert c["legs"][k]["collided"].sum() >= 1
        else:
            assert not c["legs"][k]["collided"].any()
    p = _path(wl, wl.starts, legs, allow)
    assert p["launch"]["last_kernel"] == "path_small_batch"
    _assert_path_is_chain(p, c)
    # the chain itself is the CPU oracle's chain
    q = wl.starts
    for k, targets in enumerate(legs):
        o = oracle.forward_simulate(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, q, targets, allow,
                                    call_index=BASE_CALL + k)
        for f in FIELDS:
            assert np.array_equal(p[f][k], o[f]), (k, f)
        q = o["positions"]


@pytest.mark.parametrize("small_batch", [True, False], ids=["small_on", "small_off"])
@pytest.mark.parametrize("allow", [True, False], ids=["contacts", "no_contacts"])
def test_se2_segmented_path_runs_the_throughput_kernel(fks_lib, cfg1_chains, allow, small_batch):
    """50 steps in segments of 7: the last segment of each leg is partial.  Segments do not
    change results, so the bytes are case 1's."""
    wl, legs = _cfg1_case()
    p = _path(wl, wl.starts, legs, allow, segment_steps=7, small_batch=small_batch)
    assert p["launch"]["last_kernel"] == "path"
    c = cfg1_chains[allow]
    for k in range(3):
        for f in FIELDS:
            assert np.array_equal(p[f][k], c["legs"][k][f]), (k, f)
    assert p["statistics"] == c["statistics"]
    assert p["call_index"] == BASE_CALL + 3
    # whole legs on the throughput kernel (the small-batch kernel switched off, no segments)
    if not small_batch:
        whole = _path(wl, wl.starts, legs, allow, small_batch=False)
        assert whole["launch"]["last_kernel"] == "path"
        _assert_path_is_chain(whole, c)


# ---- 2: per-particle waypoints
@pytest.mark.parametrize("allow", [True, False], ids=["contacts", "no_contacts"])
def test_per_particle_waypoints(fks_lib, allow):
    wl = W.cfg1(1.0)
    rng = np.random.default_rng(0)
    legs = [np.column_stack([rng.uniform(0.4, 3.6, 32), rng.uniform(0.4, 3.6, 32), rng.uniform(-3, 3, 32)]) for _ in range(3)]
    c = _chain(wl, wl.starts, legs, allow)
    if allow:
        assert all(c["legs"][k]["collided"].sum() > 0 for k in range(3))
    _assert_path_is_chain(_path(wl, wl.starts, legs, allow), c)


# ---- 4: more particles than resident waves (automatic segments, carry, ticket claims, early-ended legs)
def test_more_particles_than_resident_waves(fks_lib):
    wl = W.cfg1(1.0)
    sim = _sim(wl)
    try:
        sim.set_robot(wl.robot)
        n = sim.launch_geometry()["resident_waves"] + 1000
    finally:
        sim.close()
    starts = np.tile(wl.starts, (n // len(wl.starts) + 1, 1))[:n]
    legs = [wl.targets, [[0.6, 3.4, -1.0]]]
    c = _chain(wl, starts, legs, True)
    for k in range(2):
        assert c["legs"][k]["collided"].sum() > 0 and c["per_leg"][k]["controller_steps"] < n * 50
    p = _path(wl, starts, legs, True)
    assert p["launch"]["last_kernel"] == "path"
    _assert_path_is_chain(p, c)


# ---- 5: linked robot, heavy self-contact and environment contact
@pytest.mark.parametrize("segment_steps", [None, 9], ids=["whole", "segments_of_9"])
def test_linked_self_contact_path(fks_lib, segment_steps):
    wl = W.folding_arm(0.5)
    legs = [wl.targets, wl.starts[:1], wl.targets]
    c = _chain(wl, wl.starts, legs, True, segment_steps=segment_steps)
    for k in range(3):
        assert _unsuccessful(c, k) > 0
        assert c["per_leg"][k]["controller_steps"] < 16 * 100
    p = _path(wl, wl.starts, legs, True, segment_steps=segment_steps)
    whole_kernel = "path" if p["launch"]["lean"] else "path_small_batch"  # today's rule: no small-batch kernel for a lean block
    assert p["launch"]["last_kernel"] == ("path" if segment_steps else whole_kernel)
    _assert_path_is_chain(p, c)


# ---- 6, 9: linked 7-dof; shards of it
def _cfg3_case():
    wl = W.cfg3(32 / 65536)
    return wl, [wl.targets, W.CFG3_NOMINAL[None], wl.targets]


@pytest.fixture(scope="module")
def cfg3_chains(fks_lib):
    wl, legs = _cfg3_case()
    return {allow: _chain(wl, wl.starts, legs, allow) for allow in (True, False)}


@pytest.mark.parametrize("allow", [True, False], ids=["contacts", "no_contacts"])
def test_linked_7dof_path(fks_lib, cfg3_chains, allow):
    wl, legs = _cfg3_case()
    c = cfg3_chains[allow]
    for k in range(3):
        if allow:
            assert c["legs"][k]["collided"].sum() > 0 and c["per_leg"][k]["resolver_iterations"] > 0
        else:
            assert c["per_leg"][k]["controller_steps"] < 32 * wl.steps  # contacts end legs early
    _assert_path_is_chain(_path(wl, wl.starts, legs, allow), c)


def test_device_entry_shards_equal_rows_of_the_whole_path(fks_lib, cfg3_chains):
    import torch

    wl, legs = _cfg3_case()
    c = cfg3_chains[True]
    n, Wd, K = len(wl.starts), wl.robot.config_width, len(legs)
    way = torch.tensor(np.stack(legs), dtype=torch.float64, device="cuda:0").contiguous()  # [K, 1, W]
    sim = _sim(wl)
    try:
        for a, b in ((0, 11), (11, 32), (5, 6)):
            k = b - a
            d_starts = torch.tensor(wl.starts[a:b], dtype=torch.float64, device="cuda:0").contiguous()
            out = torch.zeros((K, k, Wd), dtype=torch.float64, device="cuda:0")
            coll = torch.zeros((K, k), dtype=torch.uint8, device="cuda:0")
            micro = torch.zeros((K, k), dtype=torch.int32, device="cuda:0")
            res = torch.zeros((K, k), dtype=torch.int32, device="cuda:0")
            err = torch.zeros((K, k), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            sim.set_call_index(BASE_CALL)
            sim.forward_simulate_path_device(wl.robot, d_starts.data_ptr(), k, way.data_ptr(), K, 1, a, True, out.data_ptr(),
                                             coll.data_ptr(), micro.data_ptr(), res.data_ptr(), err.data_ptr(), synchronize=True)
            assert sim.get_call_index() == BASE_CALL + K
            for leg in range(K):
                ref = c["legs"][leg]
                assert np.array_equal(out[leg].cpu().numpy(), ref["positions"][a:b]), (a, b, leg)
                assert np.array_equal(coll[leg].cpu().numpy().astype(bool), ref["collided"][a:b])
                assert np.array_equal(micro[leg].cpu().numpy().astype(np.uint32), ref["microsteps"][a:b])
                assert np.array_equal(res[leg].cpu().numpy().astype(np.uint32), ref["resolver_iterations"][a:b])
                assert np.array_equal(err[leg].cpu().numpy().astype(np.uint32), ref["error_flags"][a:b])
    finally:
        sim.close()


def test_multi_device_path_equals_single_context(fks_lib, cfg3_chains):
    from fast_kinematic_simulator_amd.simulator import MultiDeviceSimulator

    wl, legs = _cfg3_case()
    c = cfg3_chains[True]
    m = MultiDeviceSimulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed, [0, 0])
    try:
        m.set_call_index(BASE_CALL)
        r = m.forward_simulate_path_arrays(wl.robot, wl.starts, np.stack(legs), True)
        for k in range(3):
            for f in FIELDS:
                assert np.array_equal(r[f][k], c["legs"][k][f]), (k, f)
        assert m.get_statistics() == c["statistics"]
        counters = m.last_call_counters()
        for key in WORK:
            assert counters[key] == c["counters"][key], key
        assert counters["calls"] == 1
        # the multi context advanced by K: the next plain call is the chain's call BASE_CALL + 3
        nxt = m.forward_simulate_arrays(wl.robot, wl.starts, wl.targets, True)
    finally:
        m.close()
    ref = _chain(wl, wl.starts, [wl.targets], True, call=BASE_CALL + 3)["legs"][0]
    assert np.array_equal(nxt["positions"], ref["positions"])


# ---- 7: SE(3)
@pytest.mark.parametrize("allow", [True, False], ids=["contacts", "no_contacts"])
def test_se3_path(fks_lib, allow):
    wl = W.cfg4(16 / 1048576)
    legs = [wl.targets, wl.starts[:1], wl.targets]
    c = _chain(wl, wl.starts, legs, allow)
    if allow:
        assert _unsuccessful(c, 0) > 0 and _unsuccessful(c, 2) > 0
        assert c["per_leg"][1]["controller_steps"] == 16 * wl.steps
    else:
        assert c["per_leg"][0]["controller_steps"] < 16 * wl.steps and c["per_leg"][2]["controller_steps"] < 16 * wl.steps
    _assert_path_is_chain(_path(wl, wl.starts, legs, allow), c)


# ---- 8: the lean linked block (14-dof dual arm)
def test_lean_linked_path(fks_lib):
    wl = W.cfg5(6 / 1048576)
    legs = [wl.targets, wl.starts[:1]]
    c = _chain(wl, wl.starts, legs, True)
    assert c["counters"]["resolver_iterations"] > 0
    p = _path(wl, wl.starts, legs, True)
    assert p["launch"]["lean"] == 1 and p["launch"]["last_kernel"] == "path"
    _assert_path_is_chain(p, c)


# ---- 10: bookkeeping
def test_empty_batch_consumes_the_legs_call_indices(fks_lib):
    wl, legs = _cfg1_case()
    p = _path(wl, np.zeros((0, 3)), legs, True)
    assert p["positions"].shape == (3, 0, 3) and p["call_index"] == BASE_CALL + 3
    assert p["counters"]["particles"] == 0 and p["counters"]["controller_steps"] == 0


def test_refused_paths(fks_lib):
    wl, legs = _cfg1_case()
    sim = _sim(wl)
    try:
        sim.set_call_index(BASE_CALL)
        with pytest.raises(_capi.FksError) as e:
            sim.forward_simulate_path_arrays(wl.robot, wl.starts, np.zeros((0, 1, 3)), True)
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT
        sim.set_individual_jacobians(True)
        with pytest.raises(_capi.FksError) as e:
            sim.forward_simulate_path_arrays(wl.robot, wl.starts, np.stack(legs), True)
        assert e.value.status == _capi.ERR_UNSUPPORTED and "individual" in str(e.value)
        assert sim.get_call_index() == BASE_CALL  # a refused path consumes nothing
    finally:
        sim.close()


def test_path_leaves_the_specialisation_alone(fks_lib):
    """A path runs the generic path kernels: the robot's shape-specialised module is neither
    built, waited for nor launched (library defaults: specialisation on, built at the first
    plain throughput launch)."""
    from fast_kinematic_simulator_amd import make_linked_simulator

    wl, legs = _cfg1_case()
    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    try:
        sim.set_robot(wl.robot)
        sim.set_small_batch_kernel(False)  # the throughput path kernel, where a plain call would build the module
        before = sim.specialization()
        p = _path(wl, wl.starts, legs, True, sim=sim)
        after = sim.specialization()
        assert p["launch"]["last_kernel"] == "path"
        assert (after["pending"], after["launches"], after["active"]) == (before["pending"], before["launches"], before["active"])
    finally:
        sim.close()
