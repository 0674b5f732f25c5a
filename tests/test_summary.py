"""Cluster summaries on the device (fks_summarize_clusters_device, fks_summarize_clusters_ctx, the
fks_summary_<family> kernels) against the host twin fks_summarize_clusters: every comparison is of
bytes, for any conditioning.  The twin itself is held to the contract by tests/test_summary_cpu.py."""
import ctypes

import numpy as np
import pytest

import cluster_cases as CC
from fast_kinematic_simulator_amd import SUMMARY_OUTPUTS, _capi, cluster_outcomes_host, summarize_clusters_host

pytestmark = pytest.mark.gpu

# the sizes of tests/test_cluster.py: a single member, one wave's members, the staged configurations,
# the group bound
EDGE_SIZES = (0, 1, 2, 63, 64, 65, 255, 256)
GUARD = 16  # sentinel rows on either side of every output
U32, F64 = 0xA5A5A5A5, -7.25


def _sim(wl):
    from fast_kinematic_simulator_amd import make_linked_simulator

    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    sim.set_specialization(False)
    return sim


def _sizes(rng):
    sizes = list(EDGE_SIZES) + [int(v) for v in rng.integers(3, 41, 70 - len(EDGE_SIZES))]
    rng.shuffle(sizes)
    assert len(sizes) == 70
    return sizes


def _widths(robot):
    W = robot.config_width
    Wv = W if robot.robot_type == _capi.ROBOT_LINKED else (3 if robot.robot_type == _capi.ROBOT_SE2 else 6)
    return {"order": 1, "members": W, "count": 1, "begin": 1, "expectation": W, "variances": Wv, "variance": 1, "reached": 1}


def _is_u32(name):
    return name in ("order", "count", "begin", "reached")


def _device_call(sim, robot, configs, begin, labels, names, targets=None, reached_distance=0.0):
    """fks_summarize_clusters_device on torch buffers with GUARD sentinel rows around each output:
    {name: the N rows}; the sentinels are checked here"""
    import torch

    dev = torch.device("cuda", 0)
    N = int(begin[-1])
    widths = _widths(robot)
    d_q = torch.from_numpy(np.ascontiguousarray(configs)).to(dev)
    d_l = torch.from_numpy(np.ascontiguousarray(labels).view(np.int32)).to(dev)
    d_t = torch.from_numpy(np.ascontiguousarray(targets)).to(dev) if targets is not None else None
    bufs, ptrs = {}, {}
    for name in names:
        w = widths[name]
        if _is_u32(name):
            t = torch.from_numpy(np.full(((N + 2 * GUARD) * w,), U32, dtype=np.uint32).view(np.int32)).to(dev)
        else:
            t = torch.full(((N + 2 * GUARD) * w,), F64, dtype=torch.float64, device=dev)
        bufs[name] = t
        ptrs[name] = t.data_ptr() + GUARD * w * t.element_size()
    sim.summarize_clusters_device(robot, d_q.data_ptr(), begin, d_l.data_ptr(), d_t.data_ptr() if d_t is not None else 0,
                                  reached_distance, ptrs, synchronize=True)
    out = {}
    for name, t in bufs.items():
        w = widths[name]
        h = t.cpu().numpy()
        h = h.view(np.uint32) if _is_u32(name) else h
        guard = np.concatenate([h[:GUARD * w], h[(GUARD + N) * w:]])
        assert guard.size == 2 * GUARD * w and np.all(guard == (U32 if _is_u32(name) else F64)), (name, "written outside its N rows")
        out[name] = h[GUARD * w:(GUARD + N) * w]
    return out


def _same(got, ref, names, what):
    for name in names:
        a, b = np.ascontiguousarray(got[name]).reshape(-1), np.ascontiguousarray(ref[name]).reshape(-1)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name)


def _synthetic(sizes):
    """per group in turn: all one label, all distinct in descending order, every eighth out of range"""
    labels = []
    for g, n in enumerate(sizes):
        if g % 3 == 0:
            lab = np.zeros(n, dtype=np.uint32)
        elif g % 3 == 1:
            lab = np.arange(n, dtype=np.uint32)[::-1].copy()
        else:
            lab = (np.arange(n, dtype=np.uint32) * 5) % max(n // 3, 1)
        lab[::8] = np.array([n, n + 1, 0xFFFFFFFF, 0x80000000, 256, 257, n + 7, 1 << 20], dtype=np.uint32)[np.arange(0, n, 8) // 8 % 8]
        labels.append(lab)
    return labels


@pytest.mark.parametrize("name", CC.NAMES)
def test_device_equals_twin(fks_lib, name):
    wl = CC.workload(name)
    robot = wl.robot
    rng = np.random.default_rng(700 + CC.NAMES.index(name))
    sizes = _sizes(rng)
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    configs, centres = CC.draw_clumped(robot, rng, int(begin[-1]))
    groups = [configs[int(begin[g]):int(begin[g + 1])] for g in range(70)]
    D = cluster_outcomes_host(robot, [centres], 0.0, distances=True, labels=False)["distances"][0]
    mid = 0.5 * float(D[np.triu_indices(len(centres), 1)].min())
    targets = np.ascontiguousarray(centres[rng.integers(0, len(centres), 70)])
    sets = {t: cluster_outcomes_host(robot, groups, t)["labels"] for t in (0.0, mid, float("inf"))}
    sets["synthetic"] = _synthetic(sizes)
    stats = [n for n in SUMMARY_OUTPUTS if n != "reached"]
    sim = _sim(wl)
    try:
        for what, labels in sets.items():
            flat = np.concatenate(labels).astype(np.uint32)
            ref = summarize_clusters_host(robot, groups, labels)
            if what == mid:
                assert int((ref["count"] > 1).sum()) > 70, "the mid threshold made no clusters"
            if what == "synthetic":
                assert int(ref["count"].sum()) < len(flat), "no label is out of range"
            got = _device_call(sim, robot, configs, begin, flat, stats)
            _same(got, ref, stats, (name, what))
        labels = sets[mid]
        flat = np.concatenate(labels).astype(np.uint32)
        # only order and count
        ref = summarize_clusters_host(robot, groups, labels, outputs=("order", "count"))
        _same(_device_call(sim, robot, configs, begin, flat, ("order", "count")), ref, ("order", "count"), (name, "order and count"))
        # with targets: the reach is the clumps' own scale, so that some members count and some do not
        ref = summarize_clusters_host(robot, groups, labels, targets=targets, reached_distance=mid)
        assert 0 < int(ref["reached"].sum()) < int(ref["count"].sum())
        got = _device_call(sim, robot, configs, begin, flat, SUMMARY_OUTPUTS, targets=targets, reached_distance=mid)
        _same(got, ref, SUMMARY_OUTPUTS, (name, "targets"))
        got = _device_call(sim, robot, configs, begin, flat, ("reached",), targets=targets, reached_distance=mid)
        _same(got, ref, ("reached",), (name, "reached alone"))
        # the host-buffer entry
        got = sim.summarize_clusters(robot, groups, labels, targets=targets, reached_distance=mid)
        _same(got, ref, SUMMARY_OUTPUTS, (name, "host buffers"))
    finally:
        sim.close()


def test_chained_jobs_cluster_summary_jobs(fks_lib):
    """8 jobs x 32 particles of cfg1 write one buffer; clustering and summary read it in place on
    the same stream, only count and begin come down, and a second jobs call takes each non-empty
    cluster's rows of `members` as its starts by device pointer.  Its outputs equal the same two
    batches run with the host round trip (download, twins, upload) byte for byte, and the summary
    is not a call of the simulation: call index, statistics and last-call counters stay."""
    import torch

    wl = CC.workload("cfg1")
    robot, Wd = wl.robot, wl.robot.config_width
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    starts = np.ascontiguousarray(wl.starts[rng.integers(0, wl.starts.shape[0], 256)] + rng.uniform(-0.02, 0.02, (256, Wd)))
    d_starts = torch.from_numpy(starts).to(dev)
    d_target = torch.from_numpy(np.ascontiguousarray(wl.targets[:1])).to(dev)
    begin = np.arange(0, 257, 32, dtype=np.uint64)
    threshold = 0.5

    def first_jobs(out):
        return [{"d_starts": d_starts[32 * j:].data_ptr(), "n": 32, "d_targets": d_target.data_ptr(), "num_targets": 1,
                 "first_particle_id": 32 * j, "allow_contacts": True, "d_out_positions": out[32 * j:].data_ptr()} for j in range(8)]

    def second_jobs(members, count, where, out):
        """one job per non-empty cluster, in row order: its members are rows [where, where + count) of `members`"""
        rows = [r for r in range(256) if count[r] > 0]
        return [{"d_starts": members[int(where[r]):].data_ptr(), "n": int(count[r]), "d_targets": d_target.data_ptr(), "num_targets": 1,
                 "first_particle_id": 1000 + int(where[r]), "allow_contacts": True, "d_out_positions": out[int(where[r]):].data_ptr()}
                for r in rows]

    sim = _sim(wl)
    try:
        # the device route
        out1 = torch.zeros((256, Wd), dtype=torch.float64, device=dev)
        labels = torch.zeros((256,), dtype=torch.int32, device=dev)
        members = torch.zeros((256, Wd), dtype=torch.float64, device=dev)
        count = torch.zeros((256,), dtype=torch.int32, device=dev)
        where = torch.zeros((256,), dtype=torch.int32, device=dev)
        out2 = torch.zeros((256, Wd), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        sim.set_call_index(5)
        sim.forward_simulate_jobs_device(robot, first_jobs(out1), synchronize=False)
        sim.cluster_outcomes_device(robot, out1.data_ptr(), begin, threshold, 0, labels.data_ptr(), 0, synchronize=False)
        sim.summarize_clusters_device(robot, out1.data_ptr(), begin, labels.data_ptr(),
                                      d_out={"members": members.data_ptr(), "count": count.data_ptr(), "begin": where.data_ptr()},
                                      synchronize=True)
        state = (sim.get_call_index(), sim.get_statistics(), sim.last_call_counters())
        assert state[0] == 5 + 8 and state[2]["particles"] == 256
        # once more on the settled context: nothing of the simulation's moves
        sim.summarize_clusters_device(robot, out1.data_ptr(), begin, labels.data_ptr(),
                                      d_out={"members": members.data_ptr(), "count": count.data_ptr(), "begin": where.data_ptr()},
                                      synchronize=True)
        assert (sim.get_call_index(), sim.get_statistics(), sim.last_call_counters()) == state
        h_count, h_where = count.cpu().numpy(), where.cpu().numpy()  # the only downloads
        jobs2 = second_jobs(members, h_count, h_where, out2)
        assert 8 <= len(jobs2) <= 256 and sum(j["n"] for j in jobs2) == 256
        sim.forward_simulate_jobs_device(robot, jobs2, synchronize=True)
        device_route = out2.cpu().numpy()

        # the host round trip on the same context
        ref1 = torch.zeros((256, Wd), dtype=torch.float64, device=dev)
        sim.set_call_index(5)
        sim.forward_simulate_jobs_device(robot, first_jobs(ref1), synchronize=True)
        positions = ref1.cpu().numpy()
        assert positions.tobytes() == out1.cpu().numpy().tobytes()
        groups = [positions[32 * j:32 * (j + 1)] for j in range(8)]
        lab = cluster_outcomes_host(robot, groups, threshold)["labels"]
        twin = summarize_clusters_host(robot, groups, lab, outputs=("members", "count", "begin"))
        print("chained: clusters per job", [int((twin["count"][32 * j:32 * (j + 1)] > 0).sum()) for j in range(8)])
        assert twin["count"].tobytes() == h_count.view(np.uint32).tobytes() and twin["begin"].tobytes() == h_where.view(np.uint32).tobytes()
        up = torch.from_numpy(twin["members"]).to(dev)
        ref2 = torch.zeros((256, Wd), dtype=torch.float64, device=dev)
        sim.forward_simulate_jobs_device(robot, second_jobs(up, twin["count"], twin["begin"], ref2), synchronize=True)
        assert device_route.tobytes() == ref2.cpu().numpy().tobytes()
        assert np.abs(device_route - positions).max() > 0.0, "the second batch moved nothing"
    finally:
        sim.close()


def test_refusals_and_empty_calls(fks_lib):
    import torch

    wl = CC.workload("cfg1")
    robot = wl.robot
    dev = torch.device("cuda", 0)
    q = torch.zeros((600, 3), dtype=torch.float64, device=dev)
    labels = torch.zeros((600,), dtype=torch.int32, device=dev)
    tgt = torch.zeros((8, 3), dtype=torch.float64, device=dev)
    count = torch.full((600,), -7, dtype=torch.int32, device=dev)
    reached = torch.full((600,), -7, dtype=torch.int32, device=dev)
    sim = _sim(wl)
    try:
        one = (ctypes.c_uint64 * 2)(0, 1)
        asked = _capi.ClusterSummary(count=count.data_ptr())
        assert sim._lib.fks_summarize_clusters_device(sim._ctx, q.data_ptr(), one, 1, labels.data_ptr(), None, 0.0, ctypes.byref(asked),
                                                      None, 1) == _capi.ERR_NO_ROBOT
        assert sim._lib.fks_summarize_clusters_ctx(sim._ctx, None, one, 1, None, None, 0.0, ctypes.byref(asked)) == _capi.ERR_NO_ROBOT
        assert "fks_set_robot" in sim._lib.fks_get_last_error(sim._ctx).decode()
        sim.set_robot(robot)
        sim.set_call_index(3)
        before = (sim.get_call_index(), sim.get_statistics())

        def refused(begin, d_out, configs=q.data_ptr(), lab=labels.data_ptr(), targets=0, reach=1.0):
            with pytest.raises(_capi.FksError) as e:
                sim.summarize_clusters_device(robot, configs, begin, lab, targets, reach, d_out, synchronize=True)
            assert e.value.status == _capi.ERR_INVALID_ARGUMENT, e.value
            assert (sim.get_call_index(), sim.get_statistics()) == before
            return str(e.value)

        cnt = {"count": count.data_ptr()}
        assert "every pointer of the summary is NULL" in refused([0, 4], {})
        assert "null labels" in refused([0, 4], cnt, lab=0)
        assert "null configs" in refused([0, 4], cnt, configs=0)
        assert "without targets" in refused([0, 4], {"reached": reached.data_ptr()})
        assert "without reached" in refused([0, 4], cnt, targets=tgt.data_ptr())
        assert "NaN" in refused([0, 4], {"reached": reached.data_ptr()}, targets=tgt.data_ptr(), reach=float("nan"))
        assert "ascending" in refused([0, 4, 3], cnt)
        assert "FKS_MAX_CLUSTER_GROUP" in refused([0, 2, 259], cnt)
        assert "2^31" in refused([0, (1 << 31) + 1], cnt)
        st = sim._lib.fks_summarize_clusters_device(sim._ctx, q.data_ptr(), one, 1, labels.data_ptr(), None, 0.0, None, None, 1)
        assert st == _capi.ERR_INVALID_ARGUMENT and "null summary" in sim._lib.fks_get_last_error(sim._ctx).decode()
        # the host-buffer entry refuses alike
        with pytest.raises(_capi.FksError) as e:
            sim.summarize_clusters(robot, [np.zeros((257, 3))], [np.zeros(257, dtype=np.uint32)])
        assert "FKS_MAX_CLUSTER_GROUP" in str(e.value)
        # empty groups and no group at all succeed and write only what they own
        sim.summarize_clusters_device(robot, q.data_ptr(), [0, 0, 2, 2], labels.data_ptr(), d_out=cnt, synchronize=True)
        assert count.cpu().numpy()[:3].tolist() == [2, 0, -7]
        count.fill_(-7)
        sim.summarize_clusters_device(robot, 0, [0], 0, d_out=cnt, synchronize=True)
        sim.summarize_clusters_device(robot, 0, [0, 0], 0, d_out=cnt, synchronize=True)
        assert count.cpu().numpy()[:2].tolist() == [-7, -7]
        assert sim.summarize_clusters(robot, [], [])["count"].tolist() == []
        assert (sim.get_call_index(), sim.get_statistics()) == before
    finally:
        sim.close()
