"""Path, job and path-job batches on the robot's batched shape-specialised module
(fks_set_batched_specialization / fks_prepare_batched_specialization: the kernels
fks_simulate_shaped_pj and fks_simulate_shaped_pj_small).

The yardstick in every case is the same call on a second simulator with the same seed and
set_specialization(False): the generic batched kernels.  Every comparison is np.array_equal over
positions, collided, microsteps, resolver iterations and error flags of every leg of every job;
statistics, the work counters and the final call index are compared too.  Each case first
asserts on the yardstick's side that it cannot pass vacuously: some contact job collides, some
leg after the first moves particles, and the same job at another call index gives other bytes.

The file is ordered so that each robot shape's module is compiled once (the process cache keeps
it for the later cases of the same shape)."""
import os
import subprocess

import numpy as np
import pytest

from fast_kinematic_simulator_amd import workloads as W

pytestmark = pytest.mark.gpu

BASE_CALL = 5
FIELDS = ("positions", "collided", "microsteps", "resolver_iterations", "error_flags")
# what a call counts of its own work (tests/test_path_jobs.py's WORK)
WORK = ("particles", "controller_steps", "microsteps", "resolver_iterations", "sdf_bytes", "error_particles", "least_squares_rows",
        "self_collision_checks", "self_corrected_points")


def _make(wl, batched, segment_steps=None):
    from fast_kinematic_simulator_amd import make_linked_simulator

    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    if batched:
        sim.set_batched_specialization(True)
    else:
        sim.set_specialization(False)
    if segment_steps is not None:
        sim.set_segment_steps(segment_steps)
    return sim


def _way(legs, width):
    return np.stack([np.asarray(t, dtype=np.float64).reshape(-1, width) for t in legs])


def _run(sim, wl, jobs, call=BASE_CALL):
    """one path-job batch on `sim`, with everything the comparisons need"""
    Wd = wl.robot.config_width
    sim.set_robot(wl.robot)
    sim.reset_statistics()
    sim.set_call_index(call)
    r = {"jobs": sim.forward_simulate_path_jobs_arrays(wl.robot, [(s, _way(legs, Wd), a) for s, legs, a in jobs])}
    r["statistics"] = sim.get_statistics()
    r["counters"] = sim.last_call_counters()
    r["call_index"] = sim.get_call_index()
    r["kernel"] = sim.launch_info()["last_kernel"]
    return r


def _yardstick(wl, jobs, segment_steps=None, colliding=()):
    """the batch on the generic kernels (specialisation off), shown not to be vacuous"""
    sim = _make(wl, batched=False, segment_steps=segment_steps)
    try:
        probe = next(j for j, (starts, _, _) in enumerate(jobs) if len(starts) > 0)
        elsewhere = _run(sim, wl, [jobs[probe]], call=BASE_CALL + 1000)["jobs"][0]
        y = _run(sim, wl, jobs)
    finally:
        sim.close()
    assert y["kernel"] in ("path_jobs", "path_jobs_small_batch"), y["kernel"]
    assert sum(int(r["collided"].sum()) for (_, _, allow), r in zip(jobs, y["jobs"]) if allow) >= 1
    for j in colliding:
        assert jobs[j][2] and y["jobs"][j]["collided"].sum() >= 1, j
    assert any(not np.array_equal(r["positions"][k], r["positions"][k - 1]) for r in y["jobs"] for k in range(1, len(r["positions"])))
    assert not np.array_equal(elsewhere["positions"], y["jobs"][probe]["positions"])
    return y


def _assert_same(b, y, jobs):
    assert len(b["jobs"]) == len(y["jobs"]) == len(jobs)
    for j, (r, ref) in enumerate(zip(b["jobs"], y["jobs"])):
        for f in FIELDS:
            assert r[f].shape == ref[f].shape and np.array_equal(r[f], ref[f]), (j, f)
    assert b["statistics"] == y["statistics"]
    for key in WORK:
        assert b["counters"][key] == y["counters"][key], (key, b["counters"][key], y["counters"][key])
    assert b["counters"]["calls"] == 1
    assert b["counters"]["particles"] == sum(len(starts) * len(legs) for starts, legs, _ in jobs)
    assert b["call_index"] == y["call_index"] == BASE_CALL + sum(len(legs) for _, legs, _ in jobs)


# ---- SE(2): cases 1, 4, 6, 7, 8 share one compile
def _cfg1_case():
    """the mixed list of tests/test_path_jobs.py: six jobs of 3, 2, 1, 2, 2, 3 legs, one empty, one
    with a single particle, one with per-particle waypoints, both values of allow_contacts"""
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
def cfg1(fks_lib):
    wl, jobs = _cfg1_case()
    y = _yardstick(wl, jobs, segment_steps=7, colliding=(0, 3, 5))
    assert y["kernel"] == "path_jobs"
    sim = _make(wl, batched=True, segment_steps=7)
    yield wl, jobs, y, sim
    sim.close()


def test_se2_mixed_list_throughput_then_small_batch(cfg1):
    """Case 1: in segments of 7 the first batch builds the module and runs its throughput kernel
    (the short-job stale-ticket rule and the `more` rule of §4.14 in shaped code); with default
    settings the same list then fits the small-batch grid and runs the module's small kernel."""
    wl, jobs, y, sim = cfg1
    sim.set_robot(wl.robot)
    before = sim.batched_specialization()
    assert before["enabled"] and before["pending"] and not before["active"], before
    b = _run(sim, wl, jobs)
    info = sim.batched_specialization()
    print(info)
    assert b["kernel"] == "shaped_path_jobs"
    assert info["active"] and not info["pending"] and not info["failed"] and info["launches"] == 1, info
    assert info["shape"].endswith("-b") and info["shape"].startswith("t1-"), info
    assert b["jobs"][1]["positions"].shape == (2, 0, 3)
    _assert_same(b, y, jobs)
    y0 = _yardstick(wl, jobs, colliding=(0, 3, 5))  # default settings on the generic side too
    assert y0["kernel"] == "path_jobs_small_batch"
    sim.set_segment_steps(0)
    try:
        s = _run(sim, wl, jobs)
    finally:
        sim.set_segment_steps(7)
    assert s["kernel"] == "shaped_path_jobs_small_batch"
    assert sim.batched_specialization()["launches"] == 2
    _assert_same(s, y0, jobs)
    for j, (r, ref) in enumerate(zip(s["jobs"], b["jobs"])):  # segments do not change results
        for f in FIELDS:
            assert np.array_equal(r[f], ref[f]), (j, f)


def test_plain_path_and_jobs_entries_run_the_shaped_kernel(cfg1):
    """Case 4: a path of K = 3 legs and a batch of J = 4 jobs are turned into path-job form and run
    fks_simulate_shaped_pj; bytes, statistics, counters and call index are the generic entries'."""
    wl, jobs, _, sim = cfg1
    Wd = wl.robot.config_width
    starts, legs, allow = jobs[0]
    four = [(s, l[0], a) for s, l, a in (jobs[0], jobs[2], jobs[3], jobs[4])]
    ref = _make(wl, batched=False, segment_steps=7)
    out = {}
    try:
        for name, s in (("generic", ref), ("shaped", sim)):
            s.set_robot(wl.robot)
            s.reset_statistics()
            s.set_call_index(BASE_CALL)
            p = s.forward_simulate_path_arrays(wl.robot, starts, _way(legs, Wd), allow)
            pc, pk, pi = s.last_call_counters(), s.launch_info()["last_kernel"], s.get_call_index()
            j = s.forward_simulate_jobs_arrays(wl.robot, four)
            out[name] = dict(path=p, path_counters=pc, path_kernel=pk, path_index=pi, jobs=j, jobs_counters=s.last_call_counters(),
                             jobs_kernel=s.launch_info()["last_kernel"], jobs_index=s.get_call_index(), statistics=s.get_statistics())
    finally:
        ref.close()
    g, h = out["generic"], out["shaped"]
    assert (g["path_kernel"], g["jobs_kernel"]) == ("path", "jobs")
    assert (h["path_kernel"], h["jobs_kernel"]) == ("shaped_path_jobs", "shaped_path_jobs")
    assert g["path"]["collided"].sum() >= 1 and sum(int(r["collided"].sum()) for r in g["jobs"]) >= 1
    assert not np.array_equal(g["path"]["positions"][1], g["path"]["positions"][0])
    for f in FIELDS:
        assert h["path"][f].shape == g["path"][f].shape and np.array_equal(h["path"][f], g["path"][f]), f
        for k, (a_, b_) in enumerate(zip(h["jobs"], g["jobs"])):
            assert a_[f].shape == b_[f].shape and np.array_equal(a_[f], b_[f]), (k, f)
    for which in ("path_counters", "jobs_counters"):
        for key in WORK:
            assert h[which][key] == g[which][key], (which, key)
        assert h[which]["calls"] == g[which]["calls"] == 1
    assert h["path_counters"]["particles"] == 3 * len(starts) and h["jobs_counters"]["particles"] == sum(len(s) for s, _, _ in four)
    assert h["path_index"] == g["path_index"] == BASE_CALL + 3 and h["jobs_index"] == g["jobs_index"] == BASE_CALL + 7
    assert h["statistics"] == g["statistics"]


def test_laziness_and_switches(fks_lib):
    """Case 6: the module is pending after set_robot, a batch that fits the small-batch grid
    neither builds nor runs it, the switch keeps batches generic without a build, specialisation
    off clears it, and the plain module's record is untouched throughout."""
    from fast_kinematic_simulator_amd import FksError, make_linked_simulator

    wl, jobs = _cfg1_case()
    sim = _make(wl, batched=True)
    try:
        sim.set_robot(wl.robot)
        plain = sim.specialization()
        info = sim.batched_specialization()
        assert info["pending"] and not info["active"] and info["launches"] == 0, info
        b = _run(sim, wl, jobs)
        info = sim.batched_specialization()
        assert b["kernel"] == "path_jobs_small_batch"
        assert info["pending"] and not info["active"] and info["launches"] == 0, info
        sim.set_batched_specialization(False)
        sim.set_segment_steps(7)
        b = _run(sim, wl, jobs)
        info = sim.batched_specialization()
        assert b["kernel"] == "path_jobs"
        assert not info["active"] and not info["failed"] and info["launches"] == 0 and not info["enabled"], info
        sim.set_batched_specialization(True)
        assert sim.batched_specialization()["pending"]
        assert sim.specialization() == plain
        sim.set_specialization(False)
        info = sim.batched_specialization()
        assert not info["pending"] and not info["active"], info
        assert _run(sim, wl, jobs)["kernel"] == "path_jobs"
        with pytest.raises(FksError):
            sim.prepare_batched_specialization()  # needs specialisation on
    finally:
        sim.close()
    # a context with the library's defaults keeps its batches generic: the module is opt-in
    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    try:
        sim.set_segment_steps(7)
        assert _run(sim, wl, jobs)["kernel"] == "path_jobs"
        info = sim.batched_specialization()
        assert not info["enabled"] and not info["active"] and not info["pending"] and info["launches"] == 0, info
    finally:
        sim.close()


def test_failed_build_falls_back_and_is_reported(cfg1, monkeypatch, tmp_path):
    """Case 7: without the compiler helper the segmented batch keeps the generic kernel, with the
    same bytes, and the failure is reported; with the helper back the module builds and runs."""
    from fast_kinematic_simulator_amd import FksError

    wl, jobs, y, _ = cfg1
    sim = _make(wl, batched=True, segment_steps=7)
    try:
        sim.set_robot(wl.robot)
        monkeypatch.setenv("FKS_SHAPEC", str(tmp_path / "no-such-fks_shapec"))
        monkeypatch.setenv("FKS_KERNEL_CACHE", "off")
        b = _run(sim, wl, jobs)  # the lazy build fails here
        info = sim.batched_specialization()
        assert b["kernel"] == "path_jobs"
        assert info["failed"] and not info["active"] and not info["pending"], info
        assert "cannot run" in info["message"] and info["shape"].endswith("-b"), info
        assert "cannot run" in sim._lib.fks_get_last_error(sim._ctx).decode()
        _assert_same(b, y, jobs)
        with pytest.raises(FksError):
            sim.prepare_batched_specialization()
        assert sim.batched_specialization()["failed"]
        monkeypatch.delenv("FKS_SHAPEC")
        sim.prepare_batched_specialization()
        info = sim.batched_specialization()
        assert info["active"] and not info["failed"] and info["message"] == "", info
        s = _run(sim, wl, jobs)
        assert s["kernel"] == "shaped_path_jobs"
        _assert_same(s, y, jobs)
    finally:
        sim.close()


def test_device_list_0_0(cfg1):
    """Case 8: the list sharded over two contexts of device 0, each with its own batched module,
    equals the single-device generic batch byte for byte."""
    from fast_kinematic_simulator_amd.simulator import MultiDeviceSimulator

    wl, jobs, y, _ = cfg1
    Wd = wl.robot.config_width
    m = MultiDeviceSimulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed, [0, 0])
    try:
        m.set_robot(wl.robot)
        for shard in range(m.num_devices()):
            ctx = m._lib.fks_multi_device_context(m._ctx, shard)
            assert m._lib.fks_set_segment_steps(ctx, 7) == 0
        m.prepare_batched_specialization()
        for shard in range(m.num_devices()):
            assert m.device_simulator_batched_specialization(shard)["active"]
        m.set_call_index(BASE_CALL)
        r = m.forward_simulate_path_jobs_arrays(wl.robot, [(s, _way(legs, Wd), a) for s, legs, a in jobs])
        infos = [m.device_simulator_batched_specialization(shard) for shard in range(m.num_devices())]
        print(infos)
        assert all(i["launches"] == 1 for i in infos), infos  # both shards hold particles and ran the shaped kernel
        for j, (a_, b_) in enumerate(zip(r, y["jobs"])):
            for f in FIELDS:
                assert a_[f].shape == b_[f].shape and np.array_equal(a_[f], b_[f]), (j, f)
        assert m.get_statistics() == y["statistics"]
        counters = m.last_call_counters()
        for key in WORK:
            assert counters[key] == y["counters"][key], key
    finally:
        m.close()


def test_cpp_program_prepares_and_runs_the_batched_module(fks_lib):
    """Case 9: PrepareKernels(robot, batched = true), BatchedSpecializationStatus() and
    ForwardSimulateRobotsJobsAlongPaths against a second simulator with specialisation off (the
    program compares and exits non-zero on any difference)."""
    from fast_kinematic_simulator_amd.build import build_shaped_batches_test

    exe = build_shaped_batches_test()
    env = dict(os.environ)
    env.pop("FKS_SHAPEC", None)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert " 0 differences" in p.stdout, p.stdout


# ---- case 2: the 7-dof arm, the planner's edge forward and back
def test_linked_7dof_forward_and_back(fks_lib, oracle_lib):
    import oracle

    wl = W.cfg3(48 / 65536)
    forward = np.tile(np.asarray(wl.targets, dtype=np.float64).reshape(1, -1), (16, 1))
    jobs = [(wl.starts[16 * j:16 * (j + 1)], [forward, wl.starts[16 * j:16 * (j + 1)]], True) for j in range(3)]
    y = _yardstick(wl, jobs, segment_steps=3)
    sim = _make(wl, batched=True, segment_steps=3)
    try:
        b = _run(sim, wl, jobs)
        assert b["kernel"] == "shaped_path_jobs" and sim.batched_specialization()["shape"].startswith("t0-L8-J7-D7"), b["kernel"]
    finally:
        sim.close()
    _assert_same(b, y, jobs)
    # job 1 against the CPU oracle, leg by leg at its own call indices
    starts, legs, allow = jobs[1]
    q = starts
    for k, targets in enumerate(legs):
        o = oracle.forward_simulate(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, q, targets, allow,
                                    call_index=BASE_CALL + 2 + k)
        for f in FIELDS:
            assert np.array_equal(b["jobs"][1][f][k], o[f]), (k, f)
        q = o["positions"]


# ---- case 3: more particles than resident waves
def test_more_particles_than_resident_waves(fks_lib):
    """Automatic segments, ticket hand-over and a short job beside a long one, all through the
    shaped throughput kernel."""
    wl = W.cfg2(64 / 4096)
    sim = _make(wl, batched=True)
    try:
        sim.set_robot(wl.robot)
        n = sim.launch_info()["resident_waves"] + 64
        starts = np.tile(wl.starts, (n // len(wl.starts) + 1, 1))[:n]
        cut = n - 100
        nominal = np.array([[0.0, 0.9, 1.2, 0.4, 0.0, 0.3]])
        jobs = [(starts[:cut], [wl.targets, nominal], True), (starts[cut:], [wl.targets], True)]
        y = _yardstick(wl, jobs)
        assert y["kernel"] == "path_jobs"
        assert y["counters"]["controller_steps"] > 0
        b = _run(sim, wl, jobs)
        assert b["kernel"] == "shaped_path_jobs" and sim.batched_specialization()["launches"] == 1
    finally:
        sim.close()
    _assert_same(b, y, jobs)


# ---- case 5: SE(3) and the lean block
def _two_two_leg_jobs(wl):
    h = len(wl.starts) // 2
    """one job toward the target and on to a shared waypoint, one toward it and back to each particle's own start"""
    h = len(wl.starts) // 2
    forward = np.tile(np.asarray(wl.targets, dtype=np.float64).reshape(1, -1), (len(wl.starts) - h, 1))
    return [(wl.starts[:h], [wl.targets, wl.starts[:1]], True), (wl.starts[h:], [forward, wl.starts[h:]], True)]


def test_se3_shaped_batches(fks_lib):
    wl = W.cfg4(16 / 1048576)
    jobs = _two_two_leg_jobs(wl)
    y = _yardstick(wl, jobs, segment_steps=7)
    sim = _make(wl, batched=True, segment_steps=7)
    try:
        b = _run(sim, wl, jobs)
        info = sim.batched_specialization()
        assert b["kernel"] == "shaped_path_jobs" and info["shape"].startswith("t2-") and info["shape"].endswith("-b"), info
    finally:
        sim.close()
    _assert_same(b, y, jobs)


def test_lean_block_shaped_batches(fks_lib):
    wl = W.cfg5(6 / 1048576)
    jobs = _two_two_leg_jobs(wl)
    y = _yardstick(wl, jobs, segment_steps=7)
    sim = _make(wl, batched=True, segment_steps=7)
    try:
        b = _run(sim, wl, jobs)
        info = sim.batched_specialization()
        assert sim.launch_info()["lean"] == 1
        assert b["kernel"] == "shaped_path_jobs" and info["shape"].endswith("-w4-b"), info
        _assert_same(b, y, jobs)
        sim.set_segment_steps(0)  # default settings: a lean shape has no small kernel
        s = _run(sim, wl, jobs)
        assert s["kernel"] == "shaped_path_jobs"
        y0 = _yardstick(wl, jobs)
        assert y0["kernel"] == "path_jobs"
        _assert_same(s, y0, jobs)
    finally:
        sim.close()
