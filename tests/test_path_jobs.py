"""Many independent waypoint paths in one launch (fks_forward_simulate_path_jobs, the *_path_jobs
kernels).

The contract: a batch of J path jobs at call index c, job j with K_j legs, returns, byte for
byte, what the sequence of J path calls returns (job j at call index c + K_0 + ... + K_{j-1}),
its statistics and work counters are the sequence's sums, and the call index ends at c + sum K.
The reference in every case is that sequence of forward_simulate_path_arrays calls on a second
simulator with the same seed and specialisation off; every comparison is exact.  Each case first
asserts, on the sequence's side, that it cannot pass vacuously: its contact jobs collide in some
leg, its no-contact jobs never do, some leg after the first moves its particles, and the same
arguments at another call index give other bytes."""
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


def _way(legs, width):
    """a job's legs, each (1 or n, W), as the (K, 1 or n, W) array of the path entries"""
    return np.stack([np.asarray(t, dtype=np.float64).reshape(-1, width) for t in legs])


def _legs_total(jobs):
    return sum(len(legs) for _, legs, _ in jobs)


def _sequence(wl, jobs, call=BASE_CALL, **settings):
    """The jobs as forward_simulate_path_arrays calls, one after the other: per-job results,
    statistics and summed work counters.  Before them, on the same simulator, the first job
    with particles at another call index (`elsewhere`), to show that the call index matters."""
    Wd = wl.robot.config_width
    sim = _sim(wl, **settings)
    try:
        probe = next(j for j, (starts, _, _) in enumerate(jobs) if len(starts) > 0)
        first = call + sum(len(legs) for _, legs, _ in jobs[:probe])
        sim.set_call_index(first + 1000)
        elsewhere = sim.forward_simulate_path_arrays(wl.robot, jobs[probe][0], _way(jobs[probe][1], Wd), jobs[probe][2])
        sim.reset_statistics()
        out, counters, at = [], dict.fromkeys(WORK, 0), call
        for starts, legs, allow in jobs:
            sim.set_call_index(at)
            r = sim.forward_simulate_path_arrays(wl.robot, starts, _way(legs, Wd), allow)
            c = sim.last_call_counters()
            for key in WORK:
                counters[key] += c[key]
            out.append(r)
            at += len(legs)
        assert sim.get_call_index() == at
        return {"jobs": out, "statistics": sim.get_statistics(), "counters": counters, "call_index": at, "probe": probe,
                "elsewhere": elsewhere}
    finally:
        sim.close()


def _batch(wl, jobs, call=BASE_CALL, sim=None, **settings):
    Wd = wl.robot.config_width
    own = sim is None
    if own:
        sim = _sim(wl, **settings)
    try:
        sim.set_call_index(call)
        r = {"jobs": sim.forward_simulate_path_jobs_arrays(wl.robot, [(s, _way(legs, Wd), a) for s, legs, a in jobs])}
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


def _assert_batch_is_sequence(b, s, jobs):
    _assert_same_bytes(b["jobs"], s["jobs"])
    assert b["statistics"] == s["statistics"]
    for key in WORK:
        assert b["counters"][key] == s["counters"][key], (key, b["counters"][key], s["counters"][key])
    assert b["counters"]["calls"] == 1
    assert b["counters"]["particles"] == sum(len(starts) * len(legs) for starts, legs, _ in jobs)
    assert b["call_index"] == s["call_index"] == BASE_CALL + _legs_total(jobs)


def _assert_not_vacuous(s, jobs, colliding):
    """every contact job named as colliding collides in some leg, no particle of a no-contact job
    does, some leg >= 1 moves its particles, and the call index changes the bytes"""
    moved = False
    for j, (_, legs, allow) in enumerate(jobs):
        r = s["jobs"][j]
        if j in colliding:
            assert allow and r["collided"].sum() >= 1, j
        if not allow:
            assert not r["collided"].any(), j
        for k in range(1, len(legs)):
            moved = moved or not np.array_equal(r["positions"][k], r["positions"][k - 1])
    assert moved
    assert not np.array_equal(s["elsewhere"]["positions"], s["jobs"][s["probe"]]["positions"])


# ---- 1, 2: SE(2), a mixed list on the small-batch kernel, and the same list in segments
def _cfg1_case():
    wl = W.cfg1(1.0)
    rng = np.random.default_rng(0)
    per_particle = [np.column_stack([rng.uniform(0.4, 3.6, 64), rng.uniform(0.4, 3.6, 64), rng.uniform(-3, 3, 64)]) for _ in range(2)]
    a, b, c = wl.targets, [[0.6, 3.4, -1.0]], [[3.4, 0.6, 2.0]]
    jobs = [(wl.starts, [a, b, c], True),
            (wl.starts[:0], [a, b], True),
            (wl.starts[:1], [b], False),
            (np.tile(wl.starts, (2, 1)), per_particle, True),
            (wl.starts[:7], [c, b], False),
            (wl.starts, [a, b, c], True)]
    return wl, jobs


@pytest.fixture(scope="module")
def cfg1_sequence(fks_lib):
    wl, jobs = _cfg1_case()
    s = _sequence(wl, jobs)
    _assert_not_vacuous(s, jobs, colliding=(0, 3, 5))
    # the same arguments at call indices 5 and 15: the call index changes the bytes
    assert not np.array_equal(s["jobs"][0]["positions"], s["jobs"][5]["positions"])
    return s


def test_se2_mixed_path_jobs_small_batch(fks_lib, oracle_lib, cfg1_sequence):
    import oracle

    wl, jobs = _cfg1_case()
    b = _batch(wl, jobs)
    assert b["launch"]["last_kernel"] == "path_jobs_small_batch"
    assert b["jobs"][1]["positions"].shape == (2, 0, 3)
    assert not np.array_equal(b["jobs"][0]["positions"], b["jobs"][5]["positions"])  # one key per (job, leg), not per batch
    _assert_batch_is_sequence(b, cfg1_sequence, jobs)
    # a contact job against the CPU oracle: every leg from that leg's start at that leg's call index
    j = 3
    starts, legs, allow = jobs[j]
    first = BASE_CALL + _legs_total(jobs[:j])
    q = starts
    for k, targets in enumerate(legs):
        o = oracle.forward_simulate(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, q, targets, allow,
                                    call_index=first + k)
        for f in FIELDS:
            assert np.array_equal(b["jobs"][j][f][k], o[f]), (j, k, f)
        q = o["positions"]


@pytest.mark.parametrize("small_batch", [True, False], ids=["small_on", "small_off"])
def test_se2_segmented_path_jobs_run_the_throughput_kernel(fks_lib, cfg1_sequence, small_batch):
    """50 steps in segments of 7: the last segment of every leg is partial.  Segments do not
    change results, so the bytes and statistics are case 1's."""
    wl, jobs = _cfg1_case()
    b = _batch(wl, jobs, segment_steps=7, small_batch=small_batch)
    assert b["launch"]["last_kernel"] == "path_jobs"
    _assert_same_bytes(b["jobs"], cfg1_sequence["jobs"])
    assert b["statistics"] == cfg1_sequence["statistics"]
    assert b["call_index"] == BASE_CALL + 13


# ---- 3: degenerate shapes: one leg per job is a job batch, one job is a path
def test_degenerate_shapes(fks_lib, cfg1_sequence):
    wl, jobs = _cfg1_case()
    Wd = wl.robot.config_width
    one_leg = [(starts, legs[:1], allow) for starts, legs, allow in jobs]
    sim = _sim(wl)
    try:
        sim.set_call_index(BASE_CALL)
        ref = sim.forward_simulate_jobs_arrays(wl.robot, [(s, legs[0], a) for s, legs, a in one_leg])
        ref_stats, ref_index = sim.get_statistics(), sim.get_call_index()
        assert sim.launch_info()["last_kernel"] == "jobs_small_batch"
    finally:
        sim.close()
    assert sum(int(r["collided"].sum()) for r in ref) >= 1
    b = _batch(wl, one_leg)
    assert b["launch"]["last_kernel"] == "path_jobs_small_batch"
    assert len(b["jobs"]) == len(ref)
    for j, (r, x) in enumerate(zip(b["jobs"], ref)):
        for f in FIELDS:
            assert r[f].shape == (1,) + x[f].shape and np.array_equal(r[f][0], x[f]), (j, f)
    assert b["statistics"] == ref_stats and b["call_index"] == ref_index == BASE_CALL + 6

    starts, legs, allow = jobs[0]
    sim = _sim(wl)
    try:
        sim.set_call_index(BASE_CALL)
        ref = sim.forward_simulate_path_arrays(wl.robot, starts, _way(legs, Wd), allow)
        ref_stats, ref_index = sim.get_statistics(), sim.get_call_index()
    finally:
        sim.close()
    b = _batch(wl, jobs[:1])
    _assert_same_bytes(b["jobs"], [ref])
    _assert_same_bytes(b["jobs"], cfg1_sequence["jobs"][:1])
    assert b["statistics"] == ref_stats and b["call_index"] == ref_index == BASE_CALL + 3


# ---- 4: more particles than resident waves (automatic segments, carried tickets, claims across job
# and leg boundaries, the spent ticket past a short job's end while longer jobs still run, equal
# neighbours in both prefix arrays)
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
    # pieces; two empty jobs are put among them.  Legs cycle 1, 2, 3 over the jobs
    rng = np.random.default_rng(3)
    cuts = np.sort(rng.choice(np.arange(2, n), size=33, replace=False))
    bounds = [0, 1] + [int(c) for c in cuts] + [n]  # piece 0 has size 1
    bounds.insert(9, bounds[9])    # an empty job inside
    bounds.insert(20, bounds[20])  # and another
    sizes = np.diff(bounds)
    assert len(sizes) == 37 and sizes.sum() == n and (sizes == 0).sum() == 2 and (sizes == 1).sum() >= 1
    tour = [wl.targets, [[0.6, 3.4, -1.0]], [[3.4, 0.6, 2.0]]]
    jobs = [(starts[bounds[j]:bounds[j + 1]], [tour[(j + k) % 3] for k in range(j % 3 + 1)], True) for j in range(37)]
    assert {len(legs) for _, legs, _ in jobs} == {1, 2, 3}
    s = _sequence(wl, jobs)
    _assert_not_vacuous(s, jobs, colliding=())
    assert sum(int(r["collided"].sum()) for r in s["jobs"]) >= 1
    rows = sum(len(st) * len(legs) for st, legs, _ in jobs)
    assert s["counters"]["controller_steps"] < rows * 50  # some particles end a leg early
    b = _batch(wl, jobs)
    assert b["launch"]["last_kernel"] == "path_jobs"
    _assert_batch_is_sequence(b, s, jobs)


# ---- 5: linked robot, heavy self-contact beside a free-motion job
@pytest.mark.parametrize("segment_steps", [None, 9], ids=["whole", "segments_of_9"])
def test_linked_self_contact_path_jobs(fks_lib, segment_steps):
    wl = W.folding_arm(0.5)
    jobs = [(wl.starts, [wl.targets, wl.starts[:1]], True),
            (wl.starts[:3], [wl.starts[:1], wl.starts[1:2], wl.starts[2:3]], True),
            (wl.starts[:5], [wl.targets], False)]
    s = _sequence(wl, jobs, segment_steps=segment_steps)
    _assert_not_vacuous(s, jobs, colliding=(0,))
    assert s["jobs"][0]["resolver_iterations"].sum() > 0
    assert not s["jobs"][1]["collided"].any()  # the free-motion job beside the heavy one
    b = _batch(wl, jobs, segment_steps=segment_steps)
    whole_kernel = "path_jobs" if b["launch"]["lean"] else "path_jobs_small_batch"  # today's rule: no small-batch kernel for a lean block
    assert b["launch"]["last_kernel"] == ("path_jobs" if segment_steps else whole_kernel)
    _assert_batch_is_sequence(b, s, jobs)


# ---- 6, 7, 8: the planner's shape on the 7-dof arm: an edge forward and back; shards of it
def _cfg3_case():
    wl = W.cfg3(32 / 65536)
    forward = np.tile(np.asarray(wl.targets, dtype=np.float64).reshape(1, -1), (len(wl.starts), 1))
    jobs = [(wl.starts, [forward, wl.starts], True),  # to the target and back to each particle's own start
            (wl.starts[:9], [W.CFG3_NOMINAL[None]], True),
            (wl.starts[:1], [wl.targets, W.CFG3_NOMINAL[None], wl.targets], False)]
    return wl, jobs


@pytest.fixture(scope="module")
def cfg3_sequence(fks_lib):
    wl, jobs = _cfg3_case()
    s = _sequence(wl, jobs)
    _assert_not_vacuous(s, jobs, colliding=(0,))
    return s


def test_linked_7dof_forward_and_back(fks_lib, cfg3_sequence):
    wl, jobs = _cfg3_case()
    _assert_batch_is_sequence(_batch(wl, jobs), cfg3_sequence, jobs)


def test_device_entry_shards_equal_rows_of_the_whole_batch(fks_lib, cfg3_sequence):
    import torch

    wl, jobs = _cfg3_case()
    Wd = wl.robot.config_width
    dev = "cuda:0"
    sim = _sim(wl)
    try:
        # every job cut into row ranges: job 0 in three, job 1 in two, job 2 (one particle) whole or absent
        for rows in ([(0, 11), (0, 4), (0, 1)], [(11, 30), (4, 9), (0, 0)], [(30, 32), (0, 9), (0, 1)]):
            keep, d_jobs = [], []
            for (lo, hi), (starts, legs, allow) in zip(rows, jobs):
                k, K = hi - lo, len(legs)
                way = _way(legs, Wd)
                per_particle = way.shape[1] == len(starts) and len(starts) != 1
                if per_particle:
                    way = np.ascontiguousarray(way[:, lo:hi])
                t = {"starts": torch.tensor(np.asarray(starts)[lo:hi], dtype=torch.float64, device=dev).contiguous(),
                     "way": torch.tensor(way, dtype=torch.float64, device=dev).contiguous(),
                     "out": torch.zeros((K, k, Wd), dtype=torch.float64, device=dev),
                     "coll": torch.zeros((K, k), dtype=torch.uint8, device=dev),
                     "micro": torch.zeros((K, k), dtype=torch.int32, device=dev),
                     "res": torch.zeros((K, k), dtype=torch.int32, device=dev),
                     "err": torch.zeros((K, k), dtype=torch.int32, device=dev)}
                keep.append(t)
                ptr = (lambda x: x.data_ptr()) if k > 0 else (lambda x: 0)
                d_jobs.append({"d_starts": ptr(t["starts"]), "n": k, "d_waypoints": t["way"].data_ptr(), "num_legs": K,
                               "num_targets": k if per_particle else 1, "first_particle_id": lo, "allow_contacts": allow,
                               "d_out_positions": ptr(t["out"]), "d_out_collided": ptr(t["coll"]), "d_out_microsteps": ptr(t["micro"]),
                               "d_out_resolver_iterations": ptr(t["res"]), "d_out_error_flags": ptr(t["err"])})
            torch.cuda.synchronize()
            sim.set_call_index(BASE_CALL)
            sim.forward_simulate_path_jobs_device(wl.robot, d_jobs, synchronize=True)
            assert sim.get_call_index() == BASE_CALL + 6
            for j, ((lo, hi), t) in enumerate(zip(rows, keep)):
                ref = cfg3_sequence["jobs"][j]
                assert np.array_equal(t["out"].cpu().numpy(), ref["positions"][:, lo:hi]), (rows, j)
                assert np.array_equal(t["coll"].cpu().numpy().astype(bool), ref["collided"][:, lo:hi]), (rows, j)
                assert np.array_equal(t["micro"].cpu().numpy().astype(np.uint32), ref["microsteps"][:, lo:hi]), (rows, j)
                assert np.array_equal(t["res"].cpu().numpy().astype(np.uint32), ref["resolver_iterations"][:, lo:hi]), (rows, j)
                assert np.array_equal(t["err"].cpu().numpy().astype(np.uint32), ref["error_flags"][:, lo:hi]), (rows, j)
    finally:
        sim.close()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["two_shards", "three_shards"])
def test_multi_device_path_jobs_equal_single_context(fks_lib, cfg3_sequence, devices):
    """42 particles over 2 or 3 shards: a shard boundary lies inside job 0 and whole jobs are
    empty on a shard."""
    from fast_kinematic_simulator_amd.simulator import MultiDeviceSimulator

    wl, jobs = _cfg3_case()
    Wd = wl.robot.config_width
    s = cfg3_sequence
    m = MultiDeviceSimulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed, devices)
    try:
        m.set_call_index(BASE_CALL)
        r = m.forward_simulate_path_jobs_arrays(wl.robot, [(st, _way(legs, Wd), a) for st, legs, a in jobs])
        _assert_same_bytes(r, s["jobs"])
        assert m.get_statistics() == s["statistics"]
        counters = m.last_call_counters()
        for key in WORK:
            assert counters[key] == s["counters"][key], key
        assert counters["calls"] == 1
        # the multi context advanced by sum K = 6: the next plain call is the call BASE_CALL + 6
        nxt = m.forward_simulate_arrays(wl.robot, wl.starts, wl.targets, True)
    finally:
        m.close()
    sim = _sim(wl)
    try:
        sim.set_call_index(BASE_CALL + 6)
        ref = sim.forward_simulate_arrays(wl.robot, wl.starts, wl.targets, True)
    finally:
        sim.close()
    assert np.array_equal(nxt["positions"], ref["positions"])


# ---- 9: SE(3)
def test_se3_path_jobs(fks_lib):
    wl = W.cfg4(24 / 1048576)
    jobs = [(wl.starts, [wl.targets, wl.starts[:1]], True), (wl.starts[:5], [wl.targets], False)]
    s = _sequence(wl, jobs)
    _assert_not_vacuous(s, jobs, colliding=(0,))
    assert s["jobs"][0]["resolver_iterations"].sum() > 0
    _assert_batch_is_sequence(_batch(wl, jobs), s, jobs)


# ---- 10: refusals and bookkeeping on a live context
def test_refused_batches_and_bookkeeping(fks_lib):
    wl, jobs = _cfg1_case()
    Wd = wl.robot.config_width
    sim = _sim(wl)
    try:
        sim.set_robot(wl.robot)
        sim.set_call_index(BASE_CALL)
        before = sim.get_statistics()
        lib, ctx = sim._lib, sim._ctx

        def untouched():
            return sim.get_call_index() == BASE_CALL and sim.get_statistics() == before  # a refused batch consumes nothing

        def last_error():
            return lib.fks_get_last_error(ctx).decode()

        def refused(bad, status):
            with pytest.raises(_capi.FksError) as e:
                sim.forward_simulate_path_jobs_arrays(wl.robot, [(s, _way(legs, Wd), a) for s, legs, a in bad])
            assert e.value.status == status, e.value
            assert untouched()
            return str(e.value)

        starts = np.ascontiguousarray(wl.starts)
        way = _way(jobs[0][1], Wd)
        out = np.zeros((3,) + starts.shape)

        def job(n=len(starts), legs=3, nt=1, **null):
            j = _capi.PathJob(starts.ctypes.data, n, way.ctypes.data, legs, nt, 0, 1, 0, out.ctypes.data, None, None, None, None)
            for name in null:
                setattr(j, name, None)
            return j

        def refused_c(array, count, status, word):
            for entry in (lambda: lib.fks_forward_simulate_path_jobs(ctx, array, count),
                          lambda: lib.fks_forward_simulate_path_jobs_device(ctx, array, count, None, 1)):
                assert entry() == status, word
                assert word in last_error(), (word, last_error())
                assert untouched()

        # no job, too many jobs
        assert "at least one job" in refused([], _capi.ERR_INVALID_ARGUMENT)
        refused_c((_capi.PathJob * 1)(job()), 0, _capi.ERR_INVALID_ARGUMENT, "at least one job")
        many = (_capi.PathJob * 65537)(*([job(n=0)] * 65537))
        refused_c(many, 65537, _capi.ERR_INVALID_ARGUMENT, "65536 jobs")
        # a job without legs; more legs in all than records (FKS_MAX_PATH_JOB_LEGS = 65,536)
        refused_c((_capi.PathJob * 2)(job(), job(legs=0)), 2, _capi.ERR_INVALID_ARGUMENT, "job 1: a path needs at least one leg")
        refused_c((_capi.PathJob * 2)(job(n=0, legs=65536), job(n=0, legs=1)), 2, _capi.ERR_INVALID_ARGUMENT, "65536 legs")
        refused_c((_capi.PathJob * 1)(job(n=0, legs=65537)), 1, _capi.ERR_INVALID_ARGUMENT, "65536 legs")
        # waypoints per leg neither 1 nor n
        refused_c((_capi.PathJob * 2)(job(), job(n=7, nt=3)), 2, _capi.ERR_INVALID_ARGUMENT, "job 1: waypoints must hold 1 or n")
        # a job with particles and a NULL starts, waypoints or out_positions
        for missing in ("starts", "waypoints", "out_positions"):
            refused_c((_capi.PathJob * 1)(job(**{missing: True})), 1, _capi.ERR_INVALID_ARGUMENT, "null")
        # the sum of n above 2^32 - 1
        refused_c((_capi.PathJob * 2)(job(n=0xffffffff), job(n=1)), 2, _capi.ERR_INVALID_ARGUMENT, "2^32-1")
        # individual Jacobians
        sim.set_individual_jacobians(True)
        assert "individual" in refused(jobs, _capi.ERR_UNSUPPORTED)
        sim.set_individual_jacobians(False)

        # every job empty: succeeds, launches nothing, consumes the jobs' legs' call indices
        empty = [(wl.starts[:0], jobs[0][1], True), (wl.starts[:0], jobs[0][1][:1], False), (wl.starts[:0], jobs[0][1][:2], True)]
        r = sim.forward_simulate_path_jobs_arrays(wl.robot, [(s, _way(legs, Wd), a) for s, legs, a in empty])
        assert [x["positions"].shape for x in r] == [(3, 0, 3), (1, 0, 3), (2, 0, 3)]
        assert sim.get_call_index() == BASE_CALL + 6 and sim.get_statistics() == before
        assert sim.last_call_counters()["particles"] == 0
    finally:
        sim.close()

    # the longest job's legs x segments per leg must stay below 2^31 (seg_done's width): 40,000
    # controller steps in segments of one step (32,768 would do), 65,536 legs
    from fast_kinematic_simulator_amd import make_linked_simulator
    from fast_kinematic_simulator_amd.simulator import SimulatorSolverParameters

    long_solver = SimulatorSolverParameters(forward_simulation_time=40000.0 / wl.controller_frequency)
    sim = make_linked_simulator(wl.environment(), long_solver, wl.controller_frequency, wl.seed)
    try:
        sim.set_specialization(False)
        sim.set_robot(wl.robot)
        sim.set_segment_steps(1)
        sim.set_call_index(BASE_CALL)
        before = sim.get_statistics()
        starts = np.ascontiguousarray(wl.starts[:1])
        way = np.zeros((65536, 1, Wd))
        out = np.zeros((65536, 1, Wd))
        array = (_capi.PathJob * 1)(_capi.PathJob(starts.ctypes.data, 1, way.ctypes.data, 65536, 1, 0, 1, 0, out.ctypes.data))
        for entry in (lambda: sim._lib.fks_forward_simulate_path_jobs(sim._ctx, array, 1),
                      lambda: sim._lib.fks_forward_simulate_path_jobs_device(sim._ctx, array, 1, None, 1)):
            assert entry() == _capi.ERR_INVALID_ARGUMENT
            assert "2^31" in sim._lib.fks_get_last_error(sim._ctx).decode()
            assert sim.get_call_index() == BASE_CALL and sim.get_statistics() == before
    finally:
        sim.close()

    # no robot set: refused as the plain calls are
    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    try:
        array = (_capi.PathJob * 1)()
        array[0].num_legs = 1
        assert sim._lib.fks_forward_simulate_path_jobs(sim._ctx, array, 1) == _capi.ERR_NO_ROBOT
        assert sim._lib.fks_forward_simulate_path_jobs_device(sim._ctx, array, 1, None, 1) == _capi.ERR_NO_ROBOT
        assert sim.get_call_index() == 0
        # library defaults (specialisation on, built at the first plain throughput launch): a call
        # on the throughput kernel neither builds, waits for nor launches the module
        sim.set_robot(wl.robot)
        sim.set_small_batch_kernel(False)
        spec = sim.specialization()
        b = _batch(wl, jobs, sim=sim)
        after = sim.specialization()
        assert b["launch"]["last_kernel"] == "path_jobs"
        assert (after["pending"], after["launches"], after["active"]) == (spec["pending"], spec["launches"], spec["active"])
        assert sim.get_call_index() == BASE_CALL + 13
    finally:
        sim.close()
