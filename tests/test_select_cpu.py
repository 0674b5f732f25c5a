"""fks_select_states, the host twin of the selection kernels, without a GPU: the choice against the
high-precision distances of tests/hp_policy.py, the exact rules of the contract on a one-dof slider
with ==, and the draw against a plain restatement of its counter layout.

Error bound of `distance` (u = 2^-53).  The unweighted distance is the expression tree of
fks_policy_select's without the ResetPosition in front of it, so the bound counted in
tests/test_policy_cpu.py holds for it (the reset only adds wrapped terms to that count):
|error| <= c u max(1, d) + 4 u pi (sum of the wrapped terms' weights), c = D/2 + 3 (linked), 5
(SE(2)), 5.5 + 44 w1 (SE(3)).  The weight then multiplies value and error alike and the product is
rounded once more, relative u:

    |error of w d| <= w (c u max(1, d) + 4 u pi wraps) (1 + 2^-40) + u w d.

The worst measured |error| / bound of every robot is printed (and recorded in DESIGN.md 4.20).  The
states are drawn inside their limits and the continuous dofs inside (-pi, pi], where hp_policy's
ResetPosition is the identity; the queries lie up to three turns out, so the differences wrap.
hp_policy.distances takes (keys, configs) and resets the configs: the states go in as its configs,
the queries as its keys, and the distance is symmetric."""
import ctypes
import math

import numpy as np
import pytest

import cluster_cases as CC
import hp_policy
import hp_reference as hp
from fast_kinematic_simulator_amd import _capi, select_states_host, select_states_plan
from test_policy_cpu import _c, _draw

U = 2.0 ** -53
NEAR = 1e-9  # the project's near-decision margin
SIZES = (1, 63, 64, 65, 300)
N_QUERIES = 48
NONE = _capi.STATE_NONE


@pytest.fixture(scope="module")
def cases(fks_lib):
    """per robot: a pool of 300 states (a table of S states is its first S) with weights in [0.5, 2], 48
    queries and the high-precision distances [300][48], computed once"""
    out = {}
    for seed, (name, robot) in enumerate(CC.robots().items()):
        rng = np.random.default_rng(700 + seed)
        keys = _draw(robot, rng, max(SIZES), beyond=False)
        queries = CC.draw(robot, rng, N_QUERIES)
        weights = rng.uniform(0.5, 2.0, max(SIZES))
        out[name] = {"robot": robot, "keys": keys, "queries": queries, "weights": weights,
                     "hp": hp_policy.distances(robot, queries, keys)}
    return out


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name", CC.NAMES)
def test_choice_and_distance_against_high_precision(cases, name, S):
    case = cases[name]
    robot = case["robot"]
    got = select_states_host(robot, case["keys"][:S], case["queries"], weights=case["weights"][:S])
    w = hp.DEFAULT.array(case["weights"][:S])
    d = (case["hp"]["d"][:S, :] * w[:, None]).T  # [J][S] weighted, the product in high precision
    cols = np.arange(N_QUERIES)
    chosen = got["choice"].astype(np.int64)
    assert np.all(chosen < S)
    d_min = d.min(axis=1)
    near = np.array([(d[j] <= d_min[j] * (1 + hp.DEFAULT.scalar(NEAR))).sum() > 1 for j in cols])
    assert near.sum() == 0, (name, S)  # the seeded tables hold no near decision
    d_chosen = d[cols, chosen]
    assert np.all(d_chosen <= d_min * (1 + hp.DEFAULT.scalar(NEAR)))
    # distance: the derived bound
    skip = case["hp"]["near_pi"][:S, :].T[cols, chosen]
    assert skip.mean() <= 0.03
    err = np.array([abs(float(hp.DEFAULT.scalar(got["distance"][j]) - d_chosen[j])) for j in cols])
    w64 = case["weights"][:S][chosen]
    d64 = hp.to_float(case["hp"]["d"][:S, :].T[cols, chosen])
    wraps = case["hp"]["wraps"][:S, :].T[cols, chosen]
    bound = w64 * (_c(robot) * U * np.maximum(1.0, d64) + 4 * U * math.pi * wraps) * (1 + 2.0 ** -40) + U * w64 * d64
    ratio = (err / bound)[~skip]
    print(f"select_states {name} S={S}: worst |error| / bound = {ratio.max():.3f}, near pi {skip.sum()}")
    assert np.all(ratio <= 1.0), (name, S, float(ratio.max()))


def test_the_queries_wrap(cases):
    """the draw puts differences of continuous dofs outside (-pi, pi]"""
    for name, case in cases.items():
        robot = case["robot"]
        if robot.robot_type == _capi.ROBOT_SE2 or (robot.robot_type == _capi.ROBOT_LINKED and any(k[0] for k in hp_policy.dof_kinds(robot))):
            assert case["hp"]["wraps"].any(), name


# ---- the exact rules on the slider: one prismatic dof of weight 1, every distance exact
def _slider_select(keys, queries, **kw):
    return select_states_host(CC.slider(), np.asarray(keys, dtype=np.float64).reshape(-1, 1),
                              np.asarray(queries, dtype=np.float64).reshape(-1, 1), **kw)


def test_a_duplicate_key_at_a_higher_index_is_never_chosen(fks_lib):
    got = _slider_select([5.0, 2.0, 9.0, 2.0, 2.0], [2.25, 1.0, 8.0])
    assert got["choice"].tolist() == [1, 1, 2] and got["distance"].tolist() == [0.25, 1.0, 1.0]
    # an equal distance on either side of the query is a tie too
    got = _slider_select([3.0, 1.0], [2.0])
    assert got["choice"].tolist() == [0] and got["distance"].tolist() == [1.0]


def test_a_state_of_count_zero_is_skipped(fks_lib):
    got = _slider_select([5.0, 2.0, 9.0], [2.0], count=[1, 0, 1])
    assert got["choice"].tolist() == [0] and got["distance"].tolist() == [3.0]
    # without counts the same state is chosen
    assert _slider_select([5.0, 2.0, 9.0], [2.0])["choice"].tolist() == [1]


def test_a_nan_weight_never_wins(fks_lib):
    got = _slider_select([5.0, 2.0, 9.0], [2.0], weights=[1.0, np.nan, 1.0])
    assert got["choice"].tolist() == [0] and got["distance"].tolist() == [3.0]
    got = _slider_select([5.0, np.nan], [2.0])
    assert got["choice"].tolist() == [0]
    got = _slider_select([5.0], [2.0], weights=[np.nan])
    assert got["choice"].tolist() == [NONE] and got["distance"].tolist() == [np.inf]
    # an infinite distance does not win either: the scan starts from +inf under a strict <
    got = _slider_select([5.0], [2.0], weights=[np.inf])
    assert got["choice"].tolist() == [NONE] and got["distance"].tolist() == [np.inf]


def test_every_count_zero_gives_none(fks_lib):
    members = np.arange(6, dtype=np.float64).reshape(6, 1) + 1.0
    got = _slider_select([5.0, 2.0], [2.0, 7.0], num_particles=3, count=[0, 0], begin=[0, 3], members=members)
    assert got["choice"].tolist() == [NONE, NONE] and got["distance"].tolist() == [np.inf, np.inf]
    assert np.all(got["source"] == NONE)
    assert np.all(got["starts"] == 0.0) and not np.any(np.signbit(got["starts"]))


def test_null_weights_equal_unit_weights_in_every_byte(cases):
    for name, case in cases.items():
        robot = case["robot"]
        rng = np.random.default_rng(5)
        S, P = 65, 5
        count = rng.integers(0, 9, S).astype(np.uint32)
        begin = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.uint32)
        members = CC.draw(robot, rng, int(count.sum()))
        kw = dict(num_particles=P, draw_seed=77, count=count, begin=begin, members=members)
        a = select_states_host(robot, case["keys"][:S], case["queries"], **kw)
        b = select_states_host(robot, case["keys"][:S], case["queries"], weights=np.ones(S), **kw)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), (name, key)


def test_a_weight_makes_a_farther_key_win(fks_lib):
    assert _slider_select([1.0, 4.0], [0.0])["choice"].tolist() == [0]
    got = _slider_select([1.0, 4.0], [0.0], weights=[8.0, 1.0])
    assert got["choice"].tolist() == [1] and got["distance"].tolist() == [4.0]
    # the weight multiplies the distance, not the key: the key 2 x 2 would lie on the query
    got = _slider_select([2.0, 10.0], [4.0], weights=[2.0, 1.0])
    assert got["choice"].tolist() == [0] and got["distance"].tolist() == [4.0]
    got = _slider_select([2.0, 10.0], [4.0], weights=[3.5, 1.0])
    assert got["choice"].tolist() == [1] and got["distance"].tolist() == [6.0]


def test_count_equal_to_particles_copies_in_order(fks_lib):
    members = np.array([[10.0], [11.0], [12.0], [13.0], [14.0], [15.0], [16.0]])
    for seed in (0, 1, 99):
        got = _slider_select([0.0, 50.0], [49.0, 1.0], num_particles=4, draw_seed=seed, count=[3, 4], begin=[0, 3], members=members)
        assert got["choice"].tolist() == [1, 0]
        assert got["source"][0].tolist() == [3, 4, 5, 6] and got["starts"][0, :, 0].tolist() == [13.0, 14.0, 15.0, 16.0]
        assert set(got["source"][1].tolist()) <= {0, 1, 2}  # c = 3 != P: drawn
        assert got["starts"][1, :, 0].tolist() == [members[s, 0] for s in got["source"][1]]


def test_a_single_member_is_copied_to_every_start(fks_lib):
    members = np.array([[10.0], [11.0], [12.0]])
    got = _slider_select([0.0, 50.0], [49.0], num_particles=5, draw_seed=3, count=[2, 1], begin=[0, 2], members=members)
    assert got["source"].tolist() == [[2] * 5] and got["starts"][0, :, 0].tolist() == [12.0] * 5


def test_the_guard_at_the_pools_end(fks_lib):
    """begin + count one past num_member_rows: no row is read, choice and distance are still reported; the
    neighbour that ends exactly at the pool's end is drawn from"""
    members = np.array([[10.0], [11.0], [12.0], [13.0]])
    got = _slider_select([0.0, 50.0], [49.0, 1.0], num_particles=3, draw_seed=1, count=[2, 3], begin=[0, 2], members=members)
    assert got["choice"].tolist() == [1, 0] and got["distance"].tolist() == [1.0, 1.0]
    assert np.all(got["source"][0] == NONE) and np.all(got["starts"][0] == 0.0)  # 2 + 3 > 4
    assert set(got["source"][1].tolist()) <= {0, 1}
    got = _slider_select([0.0, 50.0], [49.0], num_particles=3, draw_seed=1, count=[2, 2], begin=[0, 2], members=members)
    assert set(got["source"][0].tolist()) <= {2, 3} and got["starts"][0, :, 0].tolist() == [members[s, 0] for s in got["source"][0]]


# ---- the draw
def _philox(counter, key):
    c = (ctypes.c_uint32 * 4)(*counter)
    k = (ctypes.c_uint32 * 2)(*key)
    out = (ctypes.c_uint32 * 4)()
    _capi.lib().fks_select_philox(c, k, out)
    return list(out)


def _splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def _plain_philox(counter, key):
    """Philox4x32-10 as Random123 states it"""
    c, (k0, k1) = list(counter), key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def test_the_host_philox_equals_the_random123_vectors(fks_lib):
    vectors = [(([0, 0, 0, 0], [0, 0]), [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
               (([0xFFFFFFFF] * 4, [0xFFFFFFFF, 0xFFFFFFFF]), [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
               (([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]),
                [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])]
    for (counter, key), want in vectors:
        assert _philox(counter, key) == want
        assert _plain_philox(counter, key) == want


@pytest.mark.parametrize("P", [1, 3, 4, 5, 32])
@pytest.mark.parametrize("J", [1, 9])
def test_source_equals_the_counter_layout(fks_lib, J, P):
    seed = 0x1234_5678_9ABC_DEF0 + J
    S = 6
    count = np.array([7, 2, P, 1, 11, P + 1], dtype=np.uint32)
    begin = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.uint32) + 3
    members = np.arange(3 + int(count.sum()), dtype=np.float64).reshape(-1, 1) * 0.5
    keys = np.arange(S, dtype=np.float64) * 10.0
    queries = (np.arange(J) % S) * 10.0 + 1.0  # query j is nearest state j % S
    got = _slider_select(keys, queries, num_particles=P, draw_seed=seed, count=count, begin=begin, members=members)
    key = _splitmix64(seed)
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    for j in range(J):
        i = j % S
        assert got["choice"][j] == i
        c, b = int(count[i]), int(begin[i])
        for k in range(P):
            if c == P:
                want = b + k
            else:
                r = _plain_philox([j & 0xFFFFFFFF, k >> 2, j >> 32, 0x44524157], (k0, k1))[k & 3]
                want = b + ((r * c) >> 32)
            assert got["source"][j, k] == want, (j, k)
            assert got["starts"][j, k, 0] == members[want, 0]


def test_the_draw_is_uniform_over_the_members(fks_lib):
    """J = 2,048 jobs x P = 32 starts from one state of c = 7 members at a fixed seed: each member is drawn
    65,536 / 7 = 9,362 times within five standard deviations, 5 sqrt(65,536 x 1/7 x 6/7) = 448"""
    J, P, c = 2048, 32, 7
    got = _slider_select([0.0], np.zeros(J), num_particles=P, draw_seed=20261021, count=[c], begin=[0],
                         members=np.arange(c, dtype=np.float64).reshape(c, 1), outputs=("choice", "source"))
    hist = np.bincount(got["source"].reshape(-1), minlength=c)
    print("draws per member:", hist.tolist())
    assert hist.size == c and hist.sum() == J * P
    assert np.all(np.abs(hist - 9362) <= 448), hist.tolist()
    # jobs differ, and so do the words of a block
    assert len({tuple(r) for r in got["source"].tolist()}) > J // 2


# ---- refusals that need no device
def test_select_states_refuses_malformed_arguments(fks_lib):
    robot = CC.slider()
    keys, q = np.zeros((2, 1)), np.zeros((1, 1))
    with pytest.raises(_capi.FksError):
        select_states_host(robot, np.zeros((0, 1)), q)
    with pytest.raises(_capi.FksError):  # starts without particles
        select_states_host(robot, keys, q, num_particles=0, count=[1, 1], begin=[0, 1], members=np.zeros((2, 1)), outputs=("choice", "starts"))
    with pytest.raises(_capi.FksError):  # source without members
        select_states_host(robot, keys, q, num_particles=2, count=[1, 1], begin=[0, 1], outputs=("choice", "source"))
    with pytest.raises(_capi.FksError):  # begin without count
        select_states_host(robot, keys, q, begin=[0, 1])
    with pytest.raises(_capi.FksError):  # no choice
        select_states_host(robot, keys, q, outputs=("distance",))
    with pytest.raises(_capi.FksError):
        select_states_host(robot, keys, q, num_particles=65537, count=[1, 1], begin=[0, 1], members=np.zeros((2, 1)))
    lib = _capi.lib()
    assert lib.fks_select_states(None, None, None, 0, 0, 0, None) == 1
    assert lib.fks_select_states_device(None, None, None, 0, 0, 0, None, None, 1) == 1
    assert lib.fks_select_states_ctx(None, None, None, 0, 0, 0, None) == 1
    # no query: nothing is read or written
    assert select_states_host(robot, keys, np.zeros((0, 1)))["choice"].size == 0


def test_the_plan_cuts_a_lone_query_against_600_states(fks_lib):
    """with 256 compute units the rule gives a lone query several chunks of 600 states, and one chunk when the
    table fits a workgroup's pass or the tiles alone fill the device"""
    p = select_states_plan(1, 600, 256)
    assert p == {"tile": 1, "chunk_states": 256, "chunks": 3, "groups": 3}
    assert select_states_plan(70, 70000, 256)["chunks"] > 1
    assert select_states_plan(70, 256, 256)["chunks"] == 1
    assert select_states_plan(1 << 20, 70000, 256)["chunks"] == 1
