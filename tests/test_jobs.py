"""Many independent calls in one launch (fks_forward_simulate_jobs, the *_jobs kernels).

The contract: a batch of J jobs at call index c returns, byte for byte, what the sequence of J
plain calls returns (job j at call index c + j), its statistics and work counters are the
sequence's sums, and the call index ends at c + J.  The reference in every case is that
sequence on a second simulator with the same seed; every comparison is exact.  Each case first
asserts, on the sequence's side, that its contact jobs collide and its no-contact jobs do not,
so it cannot pass on jobs in which nothing happened."""
import numpy as np
import pytest

from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd import workloads as W

pytestmark = pytest.mark.gpu

BASE_CALL = 5
FIELDS = ("positions", "collided", "microsteps", "resolver_iterations", "error_flags")
# what a call counts of its own work (not its times, and `calls`, which a batch counts once)
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


def _sequence(wl, jobs, call=BASE_CALL, **settings):
    """The jobs as plain forward_simulate_arrays calls, one after the other: per-job results,
    statistics and summed work counters."""
    sim = _sim(wl, **settings)
    try:
        out, counters = [], dict.fromkeys(WORK, 0)
        for j, (starts, targets, allow) in enumerate(jobs):
            sim.set_call_index(call + j)
            r = sim.forward_simulate_arrays(wl.robot, starts, targets, allow)
            c = sim.last_call_counters()
            for key in WORK:
                counters[key] += c[key]
            out.append(r)
        return {"jobs": out, "statistics": sim.get_statistics(), "counters": counters, "call_index": sim.get_call_index()}
    finally:
        sim.close()


def _batch(wl, jobs, call=BASE_CALL, sim=None, **settings):
    own = sim is None
    if own:
        sim = _sim(wl, **settings)
    try:
        sim.set_call_index(call)
        r = {"jobs": sim.forward_simulate_jobs_arrays(wl.robot, jobs)}
        r["statistics"] = sim.get_statistics()
        r["counters"] = sim.last_call_counters()
        r["call_index"] = sim.get_call_index()
        r["launch"] = sim.launch_info()
        return r
    finally:
        if own:
            sim.close()


def _assert_same_bytes(results, reference):
    assert len(results) == len(reference)
    for j, (r, ref) in enumerate(zip(results, reference)):
        for f in FIELDS:
            assert r[f].shape == ref[f].shape and np.array_equal(r[f], ref[f]), (j, f)


def _assert_batch_is_sequence(b, s):
    J = len(s["jobs"])
    _assert_same_bytes(b["jobs"], s["jobs"])
    assert b["statistics"] == s["statistics"]
    for key in WORK:
        assert b["counters"][key] == s["counters"][key], (key, b["counters"][key], s["counters"][key])
    assert b["counters"]["calls"] == 1
    assert b["call_index"] == s["call_index"] == BASE_CALL + J


def _assert_not_vacuous(s, jobs, colliding):
    """every contact job named as colliding collides, no particle of a no-contact job does"""
    for j, (_, _, allow) in enumerate(jobs):
        if j in colliding:
            assert allow and s["jobs"][j]["collided"].sum() >= 1, j
        if not allow:
            assert not s["jobs"][j]["collided"].any(), j


# ---- 1, 2: SE(2), mixed jobs on the small-batch jobs kernel, and the same list in segments
def _cfg1_case():
    wl = W.cfg1(1.0)
    rng = np.random.default_rng(0)
    per_particle = np.column_stack([rng.uniform(0.4, 3.6, 64), rng.uniform(0.4, 3.6, 64), rng.uniform(-3, 3, 64)])
    jobs = [(wl.starts, wl.targets, True),
            (wl.starts[:0], wl.targets, True),
            (wl.starts[:1], [[0.6, 3.4, -1.0]], False),
            (wl.starts[:7], [[3.4, 0.6, 2.0]], False),
            (np.tile(wl.starts, (2, 1)), per_particle, True),
            (wl.starts, wl.targets, True)]
    return wl, jobs


@pytest.fixture(scope="module")
def cfg1_sequence(fks_lib):
    wl, jobs = _cfg1_case()
    s = _sequence(wl, jobs)
    _assert_not_vacuous(s, jobs, colliding=(0, 4, 5))
    # the same arguments at call indices 5 and 10: the call index changes the bytes
    assert not np.array_equal(s["jobs"][0]["positions"], s["jobs"][5]["positions"])
    return s


def test_se2_mixed_jobs_small_batch(fks_lib, oracle_lib, cfg1_sequence):
    import oracle

    wl, jobs = _cfg1_case()
    b = _batch(wl, jobs)
    assert b["launch"]["last_kernel"] == "jobs_small_batch"
    assert b["jobs"][1]["positions"].shape == (0, 3)
    assert not np.array_equal(b["jobs"][0]["positions"], b["jobs"][5]["positions"])  # one key per job, not per batch
    _assert_batch_is_sequence(b, cfg1_sequence)
    for j in (0, 4):
        starts, targets, allow = jobs[j]
        o = oracle.forward_simulate(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, starts, targets, allow,
                                    call_index=BASE_CALL + j)
        for f in FIELDS:
            assert np.array_equal(b["jobs"][j][f], o[f]), (j, f)


@pytest.mark.parametrize("small_batch", [True, False], ids=["small_on", "small_off"])
def test_se2_segmented_jobs_run_the_throughput_kernel(fks_lib, cfg1_sequence, small_batch):
    """50 steps in segments of 7: the last segment is partial.  Segments do not change results,
    so the bytes are case 1's."""
    wl, jobs = _cfg1_case()
    b = _batch(wl, jobs, segment_steps=7, small_batch=small_batch)
    assert b["launch"]["last_kernel"] == "jobs"
    _assert_same_bytes(b["jobs"], cfg1_sequence["jobs"])
    assert b["statistics"] == cfg1_sequence["statistics"]
    assert b["call_index"] == BASE_CALL + 6


# ---- 3: more particles than resident waves (automatic segments, carried tickets, claims across
# job boundaries, the prefix search with equal neighbours)
def test_more_particles_than_resident_waves(fks_lib):
    wl = W.cfg1(1.0)
    sim = _sim(wl)
    try:
        sim.set_robot(wl.robot)
        n = sim.launch_geometry()["resident_waves"] + 1000
    finally:
        sim.close()
    starts = np.tile(wl.starts, (n // len(wl.starts) + 1, 1))[:n]
    # 37 jobs of uneven sizes: a first piece of size 1 and 33 distinct cuts of (1, n) make 35
    # pieces; two empty jobs are put among them
    rng = np.random.default_rng(3)
    cuts = np.sort(rng.choice(np.arange(2, n), size=33, replace=False))
    bounds = [0, 1] + [int(c) for c in cuts] + [n]  # piece 0 has size 1
    bounds.insert(9, bounds[9])    # an empty job inside
    bounds.insert(20, bounds[20])  # and another
    sizes = np.diff(bounds)
    assert len(sizes) == 37 and sizes.sum() == n and (sizes == 0).sum() == 2 and (sizes == 1).sum() >= 1
    jobs = [(starts[bounds[j]:bounds[j + 1]], wl.targets if j % 2 == 0 else [[0.6, 3.4, -1.0]], True) for j in range(37)]
    s = _sequence(wl, jobs)
    assert sum(int(r["collided"].sum()) for r in s["jobs"]) >= 1
    assert s["counters"]["controller_steps"] < n * 50  # some particles end early
    b = _batch(wl, jobs)
    assert b["launch"]["last_kernel"] == "jobs"
    _assert_batch_is_sequence(b, s)


# ---- 4: linked robot, heavy self-contact beside a free-motion job
@pytest.mark.parametrize("segment_steps", [None, 9], ids=["whole", "segments_of_9"])
def test_linked_self_contact_jobs(fks_lib, segment_steps):
    wl = W.folding_arm(0.5)
    jobs = [(wl.starts, wl.targets, True), (wl.starts[:3], wl.starts[:1], True), (wl.starts[:5], wl.targets, False)]
    s = _sequence(wl, jobs, segment_steps=segment_steps)
    _assert_not_vacuous(s, jobs, colliding=(0,))
    assert s["jobs"][0]["resolver_iterations"].sum() > 0
    assert not s["jobs"][1]["collided"].any()  # the free-motion job beside the heavy one
    b = _batch(wl, jobs, segment_steps=segment_steps)
    whole_kernel = "jobs" if b["launch"]["lean"] else "jobs_small_batch"  # today's rule: no small-batch kernel for a lean block
    assert b["launch"]["last_kernel"] == ("jobs" if segment_steps else whole_kernel)
    _assert_batch_is_sequence(b, s)


# ---- 5: linked 7-dof; shards of it
def _cfg3_case():
    wl = W.cfg3(32 / 65536)
    return wl, [(wl.starts, wl.targets, True), (wl.starts[:9], W.CFG3_NOMINAL[None], True), (wl.starts[:1], wl.targets, False)]


@pytest.fixture(scope="module")
def cfg3_sequence(fks_lib):
    wl, jobs = _cfg3_case()
    s = _sequence(wl, jobs)
    _assert_not_vacuous(s, jobs, colliding=(0,))
    assert not s["jobs"][1]["collided"].any()
    return s


def test_linked_7dof_jobs(fks_lib, cfg3_sequence):
    wl, jobs = _cfg3_case()
    _assert_batch_is_sequence(_batch(wl, jobs), cfg3_sequence)


def test_device_entry_shards_equal_rows_of_the_whole_batch(fks_lib, cfg3_sequence):
    import torch

    wl, jobs = _cfg3_case()
    Wd = wl.robot.config_width
    dev = "cuda:0"
    sim = _sim(wl)
    try:
        for a, b in ((0, 11), (11, 32), (5, 6)):
            # job 0 cut to its rows [a, b), jobs 1 and 2 whole
            rows = [(a, b), (0, 9), (0, 1)]
            keep, d_jobs = [], []
            for (lo, hi), (starts, targets, allow) in zip(rows, jobs):
                k = hi - lo
                t = {"starts": torch.tensor(np.asarray(starts)[lo:hi], dtype=torch.float64, device=dev).contiguous(),
                     "targets": torch.tensor(np.asarray(targets), dtype=torch.float64, device=dev).contiguous(),
                     "out": torch.zeros((k, Wd), dtype=torch.float64, device=dev),
                     "coll": torch.zeros(k, dtype=torch.uint8, device=dev),
                     "micro": torch.zeros(k, dtype=torch.int32, device=dev),
                     "res": torch.zeros(k, dtype=torch.int32, device=dev),
                     "err": torch.zeros(k, dtype=torch.int32, device=dev)}
                keep.append(t)
                d_jobs.append({"d_starts": t["starts"].data_ptr(), "n": k, "d_targets": t["targets"].data_ptr(), "num_targets": 1,
                               "first_particle_id": lo, "allow_contacts": allow, "d_out_positions": t["out"].data_ptr(),
                               "d_out_collided": t["coll"].data_ptr(), "d_out_microsteps": t["micro"].data_ptr(),
                               "d_out_resolver_iterations": t["res"].data_ptr(), "d_out_error_flags": t["err"].data_ptr()})
            torch.cuda.synchronize()
            sim.set_call_index(BASE_CALL)
            sim.forward_simulate_jobs_device(wl.robot, d_jobs, synchronize=True)
            assert sim.get_call_index() == BASE_CALL + 3
            for j, ((lo, hi), t) in enumerate(zip(rows, keep)):
                ref = cfg3_sequence["jobs"][j]
                assert np.array_equal(t["out"].cpu().numpy(), ref["positions"][lo:hi]), (a, b, j)
                assert np.array_equal(t["coll"].cpu().numpy().astype(bool), ref["collided"][lo:hi]), (a, b, j)
                assert np.array_equal(t["micro"].cpu().numpy().astype(np.uint32), ref["microsteps"][lo:hi]), (a, b, j)
                assert np.array_equal(t["res"].cpu().numpy().astype(np.uint32), ref["resolver_iterations"][lo:hi]), (a, b, j)
                assert np.array_equal(t["err"].cpu().numpy().astype(np.uint32), ref["error_flags"][lo:hi]), (a, b, j)
    finally:
        sim.close()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["two_shards", "three_shards"])
def test_multi_device_jobs_equal_single_context(fks_lib, cfg3_sequence, devices):
    """42 particles over 3 shards: a shard boundary lies inside job 0 and whole jobs are empty on
    a shard."""
    from fast_kinematic_simulator_amd.simulator import MultiDeviceSimulator

    wl, jobs = _cfg3_case()
    s = cfg3_sequence
    m = MultiDeviceSimulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed, devices)
    try:
        m.set_call_index(BASE_CALL)
        r = m.forward_simulate_jobs_arrays(wl.robot, jobs)
        _assert_same_bytes(r, s["jobs"])
        assert m.get_statistics() == s["statistics"]
        counters = m.last_call_counters()
        for key in WORK:
            assert counters[key] == s["counters"][key], key
        assert counters["calls"] == 1
        # the multi context advanced by J: the next plain call is the sequence's call BASE_CALL + 3
        nxt = m.forward_simulate_arrays(wl.robot, wl.starts, wl.targets, True)
    finally:
        m.close()
    ref = _sequence(wl, [(wl.starts, wl.targets, True)], call=BASE_CALL + 3)["jobs"][0]
    assert np.array_equal(nxt["positions"], ref["positions"])


# ---- 6: SE(3)
def test_se3_jobs(fks_lib):
    wl = W.cfg4(24 / 1048576)
    jobs = [(wl.starts, wl.targets, True), (wl.starts[:5], wl.targets, False), (wl.starts[:1], wl.targets, True)]
    s = _sequence(wl, jobs)
    _assert_not_vacuous(s, jobs, colliding=(0, 2))
    assert s["jobs"][0]["resolver_iterations"].sum() > 0
    _assert_batch_is_sequence(_batch(wl, jobs), s)


# ---- 7: refusals and bookkeeping on a live context
def test_refused_batches_and_bookkeeping(fks_lib, oracle_lib):
    import oracle

    wl, jobs = _cfg1_case()
    sim = _sim(wl)
    try:
        sim.set_robot(wl.robot)
        sim.set_call_index(BASE_CALL)
        before = sim.get_statistics()

        def refused(bad, status):
            with pytest.raises(_capi.FksError) as e:
                sim.forward_simulate_jobs_arrays(wl.robot, bad)
            assert e.value.status == status, e.value
            assert sim.get_call_index() == BASE_CALL and sim.get_statistics() == before  # a refused batch consumes nothing
            return str(e.value)

        refused([], _capi.ERR_INVALID_ARGUMENT)
        refused([jobs[2]] * 65537, _capi.ERR_INVALID_ARGUMENT)
        assert "job 1" in refused([jobs[0], (wl.starts[:7], wl.starts[:3], True)], _capi.ERR_INVALID_ARGUMENT)
        # a job with particles and a NULL starts, targets or out_positions, through the C entry
        starts = np.ascontiguousarray(wl.starts)
        targets = np.ascontiguousarray(np.asarray(wl.targets, dtype=np.float64).reshape(-1, 3))
        out = np.zeros_like(starts)
        for missing in ("starts", "targets", "out_positions"):
            job = _capi.Job(starts.ctypes.data, len(starts), targets.ctypes.data, 1, 0, 1, 0, out.ctypes.data, None, None, None, None)
            setattr(job, missing, None)
            array = (_capi.Job * 1)(job)
            assert sim._lib.fks_forward_simulate_jobs(sim._ctx, array, 1) == _capi.ERR_INVALID_ARGUMENT, missing
            assert sim._lib.fks_forward_simulate_jobs_device(sim._ctx, array, 1, None, 1) == _capi.ERR_INVALID_ARGUMENT, missing
            assert sim.get_call_index() == BASE_CALL and sim.get_statistics() == before
        # the sum of n above the particle limit of the host entries (2^32 - 1)
        huge = (_capi.Job * 2)(_capi.Job(starts.ctypes.data, 0xffffffff, targets.ctypes.data, 1, 0, 1, 0, out.ctypes.data),
                               _capi.Job(starts.ctypes.data, 1, targets.ctypes.data, 1, 0, 1, 0, out.ctypes.data))
        assert sim._lib.fks_forward_simulate_jobs(sim._ctx, huge, 2) == _capi.ERR_INVALID_ARGUMENT
        assert sim.get_call_index() == BASE_CALL and sim.get_statistics() == before
        sim.set_individual_jacobians(True)
        assert "individual" in refused(jobs, _capi.ERR_UNSUPPORTED)
        sim.set_individual_jacobians(False)

        # every job empty: succeeds, launches nothing, consumes the jobs' call indices
        empty = [(wl.starts[:0], wl.targets, True)] * 4
        r = sim.forward_simulate_jobs_arrays(wl.robot, empty)
        assert [x["positions"].shape for x in r] == [(0, 3)] * 4
        assert sim.get_call_index() == BASE_CALL + 4 and sim.get_statistics() == before
        assert sim.last_call_counters()["particles"] == 0
    finally:
        sim.close()

    # no robot set: refused as the plain calls are
    from fast_kinematic_simulator_amd import make_linked_simulator

    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    try:
        array = (_capi.Job * 1)()
        assert sim._lib.fks_forward_simulate_jobs(sim._ctx, array, 1) == _capi.ERR_NO_ROBOT
        assert sim._lib.fks_forward_simulate_jobs_device(sim._ctx, array, 1, None, 1) == _capi.ERR_NO_ROBOT
        # library defaults (specialisation on, built at the first plain throughput launch): a jobs
        # call on the throughput jobs kernel neither builds, waits for nor launches the module
        sim.set_robot(wl.robot)
        sim.set_small_batch_kernel(False)
        spec = sim.specialization()
        b = _batch(wl, jobs, sim=sim)
        after = sim.specialization()
        assert b["launch"]["last_kernel"] == "jobs"
        assert (after["pending"], after["launches"], after["active"]) == (spec["pending"], spec["launches"], spec["active"])
        # a plain call after a jobs call still matches the oracle at its call index
        sim.set_specialization(False)
        nxt = sim.forward_simulate_arrays(wl.robot, wl.starts, wl.targets, True)
        assert sim.get_call_index() == BASE_CALL + 7
    finally:
        sim.close()
    o = oracle.forward_simulate(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, wl.starts, wl.targets, True,
                                call_index=BASE_CALL + 6)
    for f in FIELDS:
        assert np.array_equal(nxt[f], o[f]), f
