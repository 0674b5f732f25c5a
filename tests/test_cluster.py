"""Outcome clustering on the device (fks_cluster_configs_device, fks_cluster_configs_ctx, the
fks_cluster_<family> kernels) against the host twin fks_cluster_configs: every comparison is of
bytes.  The twin itself is held to the contract by tests/test_cluster_cpu.py."""
import ctypes

import numpy as np
import pytest

import cluster_cases as CC
from fast_kinematic_simulator_amd import _capi, cluster_outcomes_host

pytestmark = pytest.mark.gpu

# one call of 70 groups: every size at which the kernel takes another path (the LDS link matrix up
# to 64, the staged configurations, one wave's columns, odd and even pair layouts, the group bound)
EDGE_SIZES = (0, 1, 2, 63, 64, 65, 255, 256)


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


def _device_call(sim, robot, configs, begin, threshold, want=(True, True, True)):
    """fks_cluster_configs_device on torch buffers: (matrices, labels, counts), None where not asked"""
    import torch

    dev = torch.device("cuda", 0)
    sizes = np.diff(begin).astype(np.int64)
    words, N, G = int((sizes * sizes).sum()), int(begin[-1]), len(begin) - 1
    d_q = torch.from_numpy(np.ascontiguousarray(configs)).to(dev)
    mats = torch.full((max(words, 1),), -7.0, dtype=torch.float64, device=dev) if want[0] else None
    labels = torch.full((max(N, 1),), -7, dtype=torch.int32, device=dev) if want[1] else None
    counts = torch.full((max(G, 1),), -7, dtype=torch.int32, device=dev) if want[2] else None
    sim.cluster_outcomes_device(robot, d_q.data_ptr(), begin, threshold, mats.data_ptr() if want[0] else 0,
                                labels.data_ptr() if want[1] else 0, counts.data_ptr() if want[2] else 0, synchronize=True)
    host = lambda t, k: None if t is None else t.cpu().numpy()[:k]
    return host(mats, words), host(labels, N), host(counts, G)


def _twin(robot, groups, threshold, distances=True, labels=True):
    r = cluster_outcomes_host(robot, groups, threshold, distances=distances, labels=labels)
    mats = np.concatenate([m.reshape(-1) for m in r["distances"]]) if distances else None
    lab = np.concatenate(r["labels"]).astype(np.uint32) if labels else None
    return mats, lab, (r["counts"] if labels else None)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", CC.NAMES)
def test_device_equals_twin(fks_lib, name):
    wl = CC.workload(name)
    robot = wl.robot
    rng = np.random.default_rng(500 + CC.NAMES.index(name))
    sizes = _sizes(rng)
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    configs, centres = CC.draw_clumped(robot, rng, int(begin[-1]))
    groups = [configs[int(begin[g]):int(begin[g + 1])] for g in range(70)]
    # a threshold between the clumps' diameter and the centres' separation
    D = cluster_outcomes_host(robot, [centres], 0.0, distances=True, labels=False)["distances"][0]
    mid = 0.5 * float(D[np.triu_indices(len(centres), 1)].min())
    sim = _sim(wl)
    try:
        for threshold in (0.0, mid, float("inf")):
            ref = _twin(robot, groups, threshold)
            if threshold == mid:
                large = [int(c) for c, n in zip(ref[2], sizes) if n >= 63]
                assert all(2 <= c <= 20 for c in large), large
            if threshold == 0.0:
                assert any(int(c) < n for c, n in zip(ref[2], sizes)), "no duplicate merged at threshold 0"
            got = _device_call(sim, robot, configs, begin, threshold)
            assert _same(got[0], ref[0]), (name, threshold, "matrices")
            assert _same(got[1].view(np.uint32), ref[1]), (name, threshold, "labels")
            assert _same(got[2].view(np.uint32), ref[2]), (name, threshold, "counts")
        ref = _twin(robot, groups, mid)
        # labels and counts alone
        got = _device_call(sim, robot, configs, begin, mid, want=(False, True, True))
        assert _same(got[1].view(np.uint32), ref[1]) and _same(got[2].view(np.uint32), ref[2])
        # the host-buffer entry
        r = sim.cluster_outcomes(robot, groups, mid, distances=True)
        assert _same(np.concatenate([m.reshape(-1) for m in r["distances"]]), ref[0])
        assert _same(np.concatenate(r["labels"]), ref[1]) and _same(r["counts"], ref[2])
        # matrices alone lift the group bound: a group of 300 beside two small ones
        big = [configs[:300], configs[300:317], configs[317:318]]
        bbegin = np.array([0, 300, 317, 318], dtype=np.uint64)
        ref = _twin(robot, big, 0.0, labels=False)
        got = _device_call(sim, robot, configs[:318], bbegin, 0.0, want=(True, False, False))
        assert _same(got[0], ref[0])
    finally:
        sim.close()


def test_chained_with_a_jobs_call(fks_lib):
    """8 jobs x 32 particles of cfg1 write one buffer; the clustering call reads it in place on the
    same stream, and is not a call of the simulation: call index, statistics and last-call counters
    stay what they were"""
    import torch

    wl = CC.workload("cfg1")
    robot, Wd = wl.robot, wl.robot.config_width
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    starts = np.ascontiguousarray(wl.starts[rng.integers(0, wl.starts.shape[0], 256)] + rng.uniform(-0.02, 0.02, (256, Wd)))
    d_starts = torch.from_numpy(starts).to(dev)
    d_target = torch.from_numpy(np.ascontiguousarray(wl.targets[:1])).to(dev)
    out = torch.zeros((256, Wd), dtype=torch.float64, device=dev)
    jobs = [{"d_starts": d_starts[32 * j:].data_ptr(), "n": 32, "d_targets": d_target.data_ptr(), "num_targets": 1,
             "first_particle_id": 32 * j, "allow_contacts": True, "d_out_positions": out[32 * j:].data_ptr()} for j in range(8)]
    begin = np.arange(0, 257, 32, dtype=np.uint64)
    labels = torch.full((256,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((8,), -7, dtype=torch.int32, device=dev)
    mats = torch.zeros((8 * 32 * 32,), dtype=torch.float64, device=dev)
    threshold = 0.5
    sim = _sim(wl)
    try:
        torch.cuda.synchronize()
        sim.set_call_index(5)
        sim.forward_simulate_jobs_device(robot, jobs, synchronize=False)
        sim.cluster_outcomes_device(robot, out.data_ptr(), begin, threshold, mats.data_ptr(), labels.data_ptr(), counts.data_ptr(),
                                    synchronize=False)
        torch.cuda.synchronize()
        state = (sim.get_call_index(), sim.get_statistics(), sim.last_call_counters())
        assert state[0] == 5 + 8 and state[2]["particles"] == 256
        positions = out.cpu().numpy()
        ref = _twin(robot, [positions[32 * j:32 * (j + 1)] for j in range(8)], threshold)
        print("chained: clusters per job", ref[2].tolist())
        assert _same(mats.cpu().numpy(), ref[0])
        assert _same(labels.cpu().numpy().view(np.uint32), ref[1]) and _same(counts.cpu().numpy().view(np.uint32), ref[2])
        # once more on the settled context: nothing of the simulation's moves, timings included
        labels.fill_(-7)
        sim.cluster_outcomes_device(robot, out.data_ptr(), begin, threshold, 0, labels.data_ptr(), counts.data_ptr(), synchronize=True)
        assert (sim.get_call_index(), sim.get_statistics(), sim.last_call_counters()) == state
        assert _same(labels.cpu().numpy().view(np.uint32), ref[1])
        sim.cluster_outcomes(robot, [positions], float("inf"))
        assert (sim.get_call_index(), sim.get_statistics(), sim.last_call_counters()) == state
    finally:
        sim.close()


def test_refusals_and_empty_calls(fks_lib):
    import torch

    wl = CC.workload("cfg1")
    robot = wl.robot
    dev = torch.device("cuda", 0)
    q = torch.zeros((600, 3), dtype=torch.float64, device=dev)
    labels = torch.full((600,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((8,), -7, dtype=torch.int32, device=dev)
    mats = torch.zeros((1 << 17,), dtype=torch.float64, device=dev)
    sim = _sim(wl)
    try:
        one = (ctypes.c_uint64 * 2)(0, 1)
        assert sim._lib.fks_cluster_configs_device(sim._ctx, q.data_ptr(), one, 1, 1.0, None, labels.data_ptr(), None, None,
                                                   1) == _capi.ERR_NO_ROBOT
        assert sim._lib.fks_cluster_configs_ctx(sim._ctx, None, one, 1, 1.0, None, None, None) == _capi.ERR_NO_ROBOT
        sim.set_robot(robot)
        sim.set_call_index(3)
        before = (sim.get_call_index(), sim.get_statistics())

        def refused(begin, threshold, want=(True, True, True), configs=q.data_ptr()):
            with pytest.raises(_capi.FksError) as e:
                sim.cluster_outcomes_device(robot, configs, begin, threshold, mats.data_ptr() if want[0] else 0,
                                            labels.data_ptr() if want[1] else 0, counts.data_ptr() if want[2] else 0, synchronize=True)
            assert e.value.status == _capi.ERR_INVALID_ARGUMENT, e.value
            assert (sim.get_call_index(), sim.get_statistics()) == before
            return str(e.value)

        assert "NaN" in refused([0, 4], float("nan"))
        assert "ascending" in refused([0, 4, 3], 1.0)
        assert "all NULL" in refused([0, 4], 1.0, want=(False, False, False))
        assert "null configs" in refused([0, 4], 1.0, configs=0)
        assert "FKS_MAX_CLUSTER_GROUP" in refused([0, 257], 1.0, want=(False, True, False))
        assert "FKS_MAX_CLUSTER_GROUP" in refused([0, 2, 259], 1.0, want=(True, False, True))
        assert "2^27" in refused([0, 11586], 1.0, want=(True, False, False))
        assert "2^31" in refused([0, (1 << 31) + 1], 1.0, want=(True, False, False))
        # the host-buffer entry refuses alike
        with pytest.raises(_capi.FksError) as e:
            sim.cluster_outcomes(robot, [np.zeros((257, 3))], 1.0)
        assert "FKS_MAX_CLUSTER_GROUP" in str(e.value)
        # empty groups and no group at all succeed and write only what they own
        sim.cluster_outcomes_device(robot, q.data_ptr(), [0, 0, 2, 2], 1.0, 0, labels.data_ptr(), counts.data_ptr(), synchronize=True)
        assert counts.cpu().numpy()[:4].tolist() == [0, 1, 0, -7] and labels.cpu().numpy()[:3].tolist() == [0, 0, -7]
        counts.fill_(-7)
        sim.cluster_outcomes_device(robot, 0, [0], 1.0, 0, 0, counts.data_ptr(), synchronize=True)
        sim.cluster_outcomes_device(robot, 0, [0, 0], 1.0, 0, 0, counts.data_ptr(), synchronize=True)
        assert counts.cpu().numpy()[:2].tolist() == [0, -7]
        assert sim.cluster_outcomes(robot, [], 1.0)["counts"].tolist() == []
        assert (sim.get_call_index(), sim.get_statistics()) == before
    finally:
        sim.close()
