"""State selection on the device (fks_select_states_device, fks_select_states_ctx, the
fks_state_select_<family> and fks_state_draw kernels) against the host twin fks_select_states: every
comparison is of bytes.  The twin itself is held to the contract by tests/test_select_cpu.py."""
import ctypes

import numpy as np
import pytest

import cluster_cases as CC
from fast_kinematic_simulator_amd import (SELECT_OUTPUTS, _capi, cluster_outcomes_host, select_states_host, select_states_plan,
                                          summarize_clusters_host)

pytestmark = pytest.mark.gpu

# (S, J, P): a single state, one wave's states, a workgroup's pass (256) and one more, tables the plan cuts
# into chunks (600 and 70,000 states); a lone query, a tile (8) less one, full and one more, several tiles
CASES = ((1, 1, 1), (63, 7, 5), (64, 8, 32), (65, 9, 1), (255, 70, 5), (256, 1, 32), (257, 8, 5), (600, 1, 5), (600, 9, 32),
         (70000, 70, 5), (70000, 1, 1))
POOL = 4096  # member rows of the cases' pool
GUARD = 16   # sentinel rows on either side of every output
U32, F64 = 0xA5A5A5A5, -7.25
NONE = _capi.STATE_NONE


def _sim(wl):
    from fast_kinematic_simulator_amd import make_linked_simulator

    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    sim.set_specialization(False)
    return sim


def _compute_units():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _spread(robot, rng, base, count):
    """count configurations: rows of `base` moved a little (an SE(3) pose in its translation alone, so it stays a pose)"""
    out = base[rng.integers(0, base.shape[0], count)].copy()
    if robot.robot_type == _capi.ROBOT_SE3:
        out[:, [3, 7, 11]] += rng.uniform(-0.05, 0.05, (count, 3))
    else:
        out += rng.uniform(-0.05, 0.05, out.shape)
    return np.ascontiguousarray(out)


def _table(robot, rng, base, S, P, chunk_states):
    """keys, weights, counts mixing 0, 1, P, below P and above P, begins anywhere in a pool of POOL rows (a few
    states end past it: the guard), and the queries' source rows"""
    keys = _spread(robot, rng, base, S)
    weights = rng.uniform(0.5, 2.0, S)
    count = rng.choice(np.array([0, 1, P, max(P - 1, 1), P + 3, 2 * P + 1], dtype=np.uint32), S)
    begin = rng.integers(0, POOL - 2 * P - 1, S).astype(np.uint32)
    begin[::7] = POOL - count[::7]            # these end exactly at the pool's end
    begin[3::11] = POOL - count[3::11] + 1    # these one row past it (an empty state among them: no state at all)
    dup = None
    if S > chunk_states:
        # one pair of duplicate keys in different chunks, with equal weights and members to draw from
        lo, hi = chunk_states // 2, S - 1 - (S - 1) % chunk_states + min(5, (S - 1) % chunk_states)
        assert lo // chunk_states != hi // chunk_states
        keys[hi] = keys[lo]
        weights[hi] = weights[lo] = 0.5
        count[lo] = count[hi] = P + 3
        begin[lo], begin[hi] = 10, 200
        dup = (lo, hi)
    return keys, weights, count, begin, dup


def _device_call(sim, robot, table, queries, P, seed, names, W):
    """fks_select_states_device on torch buffers with GUARD sentinel rows around each output: {name: its rows};
    the sentinels are checked here.  table: a dict of host arrays (None: not given)."""
    import torch

    dev = torch.device("cuda", 0)
    J = queries.shape[0]

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

    d_table = {k: up(v) for k, v in table.items()}
    d_q = up(queries)
    widths = {"choice": 1, "distance": 1, "starts": P * W, "source": P}
    bufs, ptrs = {}, {}
    for name in names:
        w = widths[name]
        if name in ("choice", "source"):
            t = torch.from_numpy(np.full(((J + 2 * GUARD) * w,), U32, dtype=np.uint32).view(np.int32)).to(dev)
        else:
            t = torch.full(((J + 2 * GUARD) * w,), F64, dtype=torch.float64, device=dev)
        bufs[name] = t
        ptrs[name] = t.data_ptr() + GUARD * w * t.element_size()
    sim.select_states_device(robot, {k: v.data_ptr() for k, v in d_table.items() if v is not None}, table["keys"].shape[0],
                             d_q.data_ptr(), J, P, seed, ptrs,
                             num_member_rows=0 if table.get("members") is None else table["members"].shape[0], synchronize=True)
    out = {}
    for name, t in bufs.items():
        w = widths[name]
        h = t.cpu().numpy()
        h = h.view(np.uint32) if name in ("choice", "source") else h
        guard = np.concatenate([h[:GUARD * w], h[(GUARD + J) * w:]])
        assert guard.size == 2 * GUARD * w and np.all(guard == (U32 if h.dtype == np.uint32 else F64)), (name, "written outside its J rows")
        out[name] = h[GUARD * w:(GUARD + J) * w]
    return out


def _same(got, ref, names, what):
    for name in names:
        a, b = np.ascontiguousarray(got[name]).reshape(-1), np.ascontiguousarray(ref[name]).reshape(-1)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name)


def test_the_plan_cuts_600_and_70000_states(fks_lib):
    """the cases above reach the multi-chunk path on this device and on one of 256 compute units"""
    for cus in (_compute_units(), 256):
        assert select_states_plan(1, 600, cus)["chunks"] > 1
        assert select_states_plan(9, 600, cus)["chunks"] > 1
        assert select_states_plan(70, 70000, cus)["chunks"] > 1
        assert select_states_plan(1, 70000, cus)["chunks"] > 1
        assert select_states_plan(70, 255, cus)["chunks"] == 1


@pytest.mark.parametrize("name", CC.NAMES)
def test_device_equals_twin(fks_lib, name):
    wl = CC.workload(name)
    robot, W = wl.robot, wl.robot.config_width
    rng = np.random.default_rng(900 + CC.NAMES.index(name))
    base = CC.draw(robot, rng, 256)
    members = _spread(robot, rng, base, POOL)
    cus = _compute_units()
    sim = _sim(wl)
    try:
        seen = {"drawn": False, "in order": False, "guarded": False}
        for S, J, P in CASES:
            plan = select_states_plan(J, S, cus)
            keys, weights, count, begin, dup = _table(robot, rng, base, S, P, plan["chunk_states"])
            queries = _spread(robot, rng, base, J)
            if dup:
                queries[J - 1] = keys[dup[0]]  # on the duplicated key: both copies tie
            table = {"keys": keys, "weights": weights, "count": count, "begin": begin, "members": members}
            seed = 1000 * S + J
            ref = select_states_host(robot, keys, queries, P, seed, weights=weights, count=count, begin=begin, members=members)
            if dup:
                assert plan["chunks"] > 1 and ref["choice"][J - 1] == dup[0], (name, S, J)
            chosen = ref["choice"][ref["choice"] != NONE]
            seen["drawn"] |= bool(np.any(count[chosen] != P))
            seen["in order"] |= bool(np.any(count[chosen] == P))
            seen["guarded"] |= bool(np.any(np.all(ref["source"] == NONE, axis=1) & (ref["choice"] != NONE)))
            got = _device_call(sim, robot, table, queries, P, seed, SELECT_OUTPUTS, W)
            _same(got, ref, SELECT_OUTPUTS, (name, S, J, P))
        assert all(seen.values()), ("the cases decide too little", seen)
        # the other calls on one table of several chunks
        S, J, P = 600, 9, 5
        keys, weights, count, begin, _ = _table(robot, rng, base, S, P, select_states_plan(J, S, cus)["chunk_states"])
        queries = _spread(robot, rng, base, J)
        # selection only: no count (an empty state is then a state), no draw
        ref = select_states_host(robot, keys, queries, weights=weights)
        got = _device_call(sim, robot, {"keys": keys, "weights": weights}, queries, 0, 0, ("choice", "distance"), W)
        _same(got, ref, ("choice", "distance"), (name, "selection only"))
        # without weights, choice alone
        ref = select_states_host(robot, keys, queries, outputs=("choice",))
        _same(_device_call(sim, robot, {"keys": keys}, queries, 0, 0, ("choice",), W), ref, ("choice",), (name, "choice alone"))
        # source without starts
        table = {"keys": keys, "weights": weights, "count": count, "begin": begin, "members": members}
        ref = select_states_host(robot, keys, queries, P, 4, weights=weights, count=count, begin=begin, members=members)
        got = _device_call(sim, robot, table, queries, P, 4, ("choice", "source"), W)
        _same(got, ref, ("choice", "source"), (name, "source without starts"))
        # the host-buffer entry
        got = sim.select_states(robot, keys, queries, P, 4, weights=weights, count=count, begin=begin, members=members)
        _same(got, ref, SELECT_OUTPUTS, (name, "host buffers"))
        got = sim.select_states(robot, keys, queries, weights=weights)
        _same(got, select_states_host(robot, keys, queries, weights=weights), ("choice", "distance"), (name, "host buffers, selection only"))
    finally:
        sim.close()


def test_chained_select_feeds_jobs(fks_lib):
    """8 jobs x 32 particles of cfg1 write into a pool behind 64 rows of an earlier batch; clustering and
    summary append the batch's child states at group_begin[0] = 64; the selection then finds the nearest
    state of the whole pool for 8 new targets and writes each job's 32 starts, which a second jobs call
    reads by device pointer.  One stream, only `choice` comes down.  The outputs equal the same sequence
    run with the host round trip (download, the three twins, upload) byte for byte, and the selection is
    not a call of the simulation: call index, statistics and last-call counters stay."""
    import torch

    wl = CC.workload("cfg1")
    robot, Wd = wl.robot, wl.robot.config_width
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    USED, ROWS = 64, 64 + 256
    starts = np.ascontiguousarray(wl.starts[rng.integers(0, wl.starts.shape[0], 256)] + rng.uniform(-0.02, 0.02, (256, Wd)))
    new_targets = np.ascontiguousarray(wl.targets[rng.integers(0, wl.targets.shape[0], 8)] + rng.uniform(-0.3, 0.3, (8, Wd)))
    # the earlier batch: one state of 32 members at row 0, far from no target in particular; rows 1 .. 63 are empty clusters
    earlier = {"members": np.full((USED, Wd), 0.5), "count": np.zeros(USED, dtype=np.uint32), "begin": np.zeros(USED, dtype=np.uint32),
               "expectation": np.zeros((USED, Wd))}
    earlier["members"][:32] = starts[:32]
    earlier["count"][0] = 32
    earlier["expectation"][0] = starts[0]
    d_starts = torch.from_numpy(starts).to(dev)
    d_target = torch.from_numpy(np.ascontiguousarray(wl.targets[:1])).to(dev)
    d_new = torch.from_numpy(new_targets).to(dev)
    begin = (USED + np.arange(0, 257, 32)).astype(np.uint64)
    threshold, seed, P = 0.5, 99, 32

    def first_jobs(out):
        return [{"d_starts": d_starts[32 * j:].data_ptr(), "n": 32, "d_targets": d_target.data_ptr(), "num_targets": 1,
                 "first_particle_id": 32 * j, "allow_contacts": True, "d_out_positions": out[USED + 32 * j:].data_ptr()} for j in range(8)]

    def second_jobs(sel_starts, out):
        return [{"d_starts": sel_starts[j].data_ptr(), "n": P, "d_targets": d_new[j:].data_ptr(), "num_targets": 1,
                 "first_particle_id": 1000 + P * j, "allow_contacts": True, "d_out_positions": out[P * j:].data_ptr()} for j in range(8)]

    def pool(name, dtype):
        host = np.zeros((ROWS,) + earlier[name].shape[1:], dtype=earlier[name].dtype)
        host[:USED] = earlier[name]
        return torch.from_numpy(host.view(np.int32) if dtype == np.uint32 else host).to(dev)

    sim = _sim(wl)
    try:
        # the device route
        outs = torch.zeros((ROWS, Wd), dtype=torch.float64, device=dev)
        labels = torch.zeros((ROWS,), dtype=torch.int32, device=dev)
        members, expectation = pool("members", np.float64), pool("expectation", np.float64)
        count, where = pool("count", np.uint32), pool("begin", np.uint32)
        choice = torch.full((8,), -1, dtype=torch.int32, device=dev)
        sel_starts = torch.zeros((8, P, Wd), dtype=torch.float64, device=dev)
        out2 = torch.zeros((8 * P, Wd), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        sim.set_call_index(5)
        sim.forward_simulate_jobs_device(robot, first_jobs(outs), synchronize=False)
        sim.cluster_outcomes_device(robot, outs.data_ptr(), begin, threshold, 0, labels.data_ptr(), 0, synchronize=False)
        sim.summarize_clusters_device(robot, outs.data_ptr(), begin, labels.data_ptr(),
                                      d_out={"members": members.data_ptr(), "count": count.data_ptr(), "begin": where.data_ptr(),
                                             "expectation": expectation.data_ptr()}, synchronize=True)
        state = (sim.get_call_index(), sim.get_statistics(), sim.last_call_counters())
        assert state[0] == 5 + 8 and state[2]["particles"] == 256
        d_table = {"keys": expectation.data_ptr(), "count": count.data_ptr(), "begin": where.data_ptr(), "members": members.data_ptr()}
        d_out = {"choice": choice.data_ptr(), "starts": sel_starts.data_ptr()}
        sim.select_states_device(robot, d_table, ROWS, d_new.data_ptr(), 8, P, seed, d_out, num_member_rows=ROWS, synchronize=True)
        assert (sim.get_call_index(), sim.get_statistics(), sim.last_call_counters()) == state
        sim.select_states_device(robot, d_table, ROWS, d_new.data_ptr(), 8, P, seed, d_out, num_member_rows=ROWS, synchronize=False)
        sim.forward_simulate_jobs_device(robot, second_jobs(sel_starts, out2), synchronize=True)
        assert sim.get_call_index() == 5 + 8 + 8
        h_choice = choice.cpu().numpy().view(np.uint32)  # the only download of the route
        device_route = out2.cpu().numpy()

        # the host round trip on the same context
        ref1 = torch.zeros((ROWS, Wd), dtype=torch.float64, device=dev)
        sim.set_call_index(5)
        sim.forward_simulate_jobs_device(robot, first_jobs(ref1), synchronize=True)
        positions = ref1.cpu().numpy()[USED:]
        assert positions.tobytes() == outs.cpu().numpy()[USED:].tobytes()
        groups = [positions[32 * j:32 * (j + 1)] for j in range(8)]
        lab = cluster_outcomes_host(robot, groups, threshold)["labels"]
        twin = summarize_clusters_host(robot, groups, lab, outputs=("members", "count", "begin", "expectation"))
        host = {"members": np.concatenate([earlier["members"], twin["members"]]),
                "count": np.concatenate([earlier["count"], twin["count"]]),
                "begin": np.concatenate([earlier["begin"], twin["begin"] + np.uint32(USED)]),
                "expectation": np.concatenate([earlier["expectation"], twin["expectation"]])}
        assert host["count"].tobytes() == count.cpu().numpy().view(np.uint32).tobytes()
        assert host["begin"].tobytes() == where.cpu().numpy().view(np.uint32).tobytes()
        assert host["members"].tobytes() == members.cpu().numpy().tobytes() and host["expectation"].tobytes() == expectation.cpu().numpy().tobytes()
        sel = select_states_host(robot, host["expectation"], new_targets, P, seed, count=host["count"], begin=host["begin"],
                                 members=host["members"])
        print("chained: choices", sel["choice"].tolist(), "their counts", host["count"][sel["choice"]].tolist())
        assert sel["choice"].tobytes() == h_choice.tobytes() and np.all(sel["choice"] != NONE)
        assert sel["starts"].tobytes() == sel_starts.cpu().numpy().tobytes()
        assert np.any(host["count"][sel["choice"]] != P), "every chosen state had exactly P members: nothing was drawn"
        up = torch.from_numpy(sel["starts"]).to(dev)
        ref2 = torch.zeros((8 * P, Wd), dtype=torch.float64, device=dev)
        sim.forward_simulate_jobs_device(robot, second_jobs(up, ref2), synchronize=True)
        assert device_route.tobytes() == ref2.cpu().numpy().tobytes()
        assert np.abs(device_route - sel["starts"].reshape(-1, Wd)).max() > 0.0, "the second batch moved nothing"
    finally:
        sim.close()


def test_refusals_and_empty_calls(fks_lib):
    import torch

    wl = CC.workload("cfg1")
    robot = wl.robot
    dev = torch.device("cuda", 0)
    keys = torch.zeros((600, 3), dtype=torch.float64, device=dev)
    words = torch.ones((600,), dtype=torch.int32, device=dev)
    choice = torch.full((16,), -7, dtype=torch.int32, device=dev)
    rows = torch.zeros((16 * 4, 3), dtype=torch.float64, device=dev)
    sim = _sim(wl)
    try:
        t = _capi.StateTable(keys=keys.data_ptr(), num_states=600)
        o = _capi.StateSelection(choice=choice.data_ptr())
        assert sim._lib.fks_select_states_device(sim._ctx, ctypes.byref(t), keys.data_ptr(), 4, 0, 0, ctypes.byref(o), None,
                                                 1) == _capi.ERR_NO_ROBOT
        assert sim._lib.fks_select_states_ctx(sim._ctx, ctypes.byref(t), None, 4, 0, 0, ctypes.byref(o)) == _capi.ERR_NO_ROBOT
        assert "fks_set_robot" in sim._lib.fks_get_last_error(sim._ctx).decode()
        sim.set_robot(robot)
        sim.set_call_index(3)
        before = (sim.get_call_index(), sim.get_statistics())
        full = {"keys": keys.data_ptr(), "count": words.data_ptr(), "begin": words.data_ptr(), "members": keys.data_ptr()}
        plain = {"keys": keys.data_ptr()}
        ch = {"choice": choice.data_ptr()}
        st = {"choice": choice.data_ptr(), "starts": rows.data_ptr()}
        so = {"choice": choice.data_ptr(), "source": words.data_ptr()}

        def refused(table, S, J, P, d_out, queries=keys.data_ptr()):
            with pytest.raises(_capi.FksError) as e:
                sim.select_states_device(robot, table, S, queries, J, P, 0, d_out, num_member_rows=600, synchronize=True)
            assert e.value.status == _capi.ERR_INVALID_ARGUMENT, e.value
            assert (sim.get_call_index(), sim.get_statistics()) == before
            return str(e.value)

        assert "null keys" in refused({}, 600, 4, 0, ch)
        assert "at least one state" in refused(plain, 0, 4, 0, ch)
        assert "2^30" in refused(plain, (1 << 30) + 1, 4, 0, ch)
        assert "null choice" in refused(plain, 600, 4, 0, {})
        assert "null queries" in refused(plain, 600, 4, 0, ch, queries=0)
        assert "num_particles == 0" in refused(full, 600, 4, 0, st)
        assert "num_particles == 0" in refused(full, 600, 4, 0, so)
        for missing in ("count", "begin", "members"):
            table = {k: v for k, v in full.items() if k != missing and not (missing == "count" and k == "begin")}
            assert "without count, begin and members" in refused(table, 600, 4, 4, st)
            assert "without count, begin and members" in refused(table, 600, 4, 4, so)
        assert "begin is given without count" in refused({"keys": keys.data_ptr(), "begin": words.data_ptr()}, 600, 4, 0, ch)
        assert "2^20" in refused(plain, 600, (1 << 20) + 1, 0, ch)
        assert "65536" in refused(full, 600, 4, 65537, st)
        assert "2^31" in refused(full, 600, 1 << 20, 2049, st)
        for table, out, text in ((None, o, "null state table"), (t, None, "null selection")):
            code = sim._lib.fks_select_states_device(sim._ctx, ctypes.byref(table) if table else None, keys.data_ptr(), 4, 0, 0,
                                                     ctypes.byref(out) if out else None, None, 1)
            assert code == _capi.ERR_INVALID_ARGUMENT and text in sim._lib.fks_get_last_error(sim._ctx).decode()
        # the host-buffer entry refuses alike
        with pytest.raises(_capi.FksError) as e:
            sim.select_states(robot, np.zeros((2, 3)), np.zeros((1, 3)), begin=[0, 1])
        assert "begin is given without count" in str(e.value)
        # no query: nothing is launched or written
        sim.select_states_device(robot, plain, 600, 0, 0, 0, 0, {}, synchronize=True)
        sim.select_states_device(robot, plain, 600, keys.data_ptr(), 0, 4, 0, ch, synchronize=True)
        assert choice.cpu().numpy().tolist() == [-7] * 16
        assert sim.select_states(robot, np.zeros((2, 3)), np.zeros((0, 3)))["choice"].tolist() == []
        assert (sim.get_call_index(), sim.get_statistics()) == before
    finally:
        sim.close()
