"""fks_policy_select, the host twin of the policy kernels' selection, without a GPU: against the
high-precision selection of tests/hp_policy.py, the exact rules of the contract with ==, and the
refusals that need no device.

Error bounds of out_distance, counted operation by operation (u = 2^-53, one rounding of a
float64 operation; inputs are exact float64 values; first order, times 1 + 2^-40 for the rest):

  linked, D dofs.  delta_k = key_k - p_k (u), e_k = w_k |delta_k| (u) -> 2u; e_k^2 (u) -> 5u; the
    sum of D non-negative terms, D - 1 roundings of at most u x total -> (D + 4) u; the square root
    halves it and rounds once -> (D/2 + 3) u relative:   c = D/2 + 3.
  SE(2).  dx, dy (u each), squares (u) -> 3u; the sum (u) -> 4u; sqrt -> 2u + u = 3u; x w0 (u) ->
    4u on the first term; |wrap(delta theta)| x w1 -> 2u on the second; the final sum (u):   c = 5.
  SE(3).  w0 ||delta t||: three differences (u), squares (u), two sums (2u) -> 5u, sqrt -> 3.5u,
    x w0 -> 4.5u.  The angle: an entry of R^T R' is a 3-term dot product of unit rows, absolute
    error 3u; cos = (trace - 1) / 2 from three entries (9u) and three sums of magnitude <= 3 (9u),
    halved -> 9u; a component of the skew vector (3u + 3u + 2u) / 2 = 4u, its norm s
    4 sqrt(3) u + 2.5u < 9.5u; theta = atan2(s, cos) moves by at most sqrt(9^2 + 9.5^2) u < 13.1u
    and is rounded within 2 ulp of a value below 4 -> 8u; w = vee (theta / s) and its norm are
    theta (1 +- 7u) -> 7 pi u < 22u: 43.1u absolute on the angle, x w1 (u on the product), and the
    final sum (u):   |error| <= 5.5u d + 44u w1, so c = 5.5 + 44 w1 with max(1, d).
  A wrapped term (a continuous dof's or the SE(2) angle's ResetPosition, and the wrap of a
  difference) is exact modulo the float64 2 pi, which differs from 2 pi by 2.45e-16 per turn: the
  contract's 4u pi per wrapped term, weighted by the term's weight as it enters the distance
  (d is 1-Lipschitz in every weighted term).

The bound is c u max(1, d) + 4 u pi (sum of the wrapped terms' weights).  The worst measured
ratio |error| / bound of every robot is printed (and recorded in DESIGN.md 4.17)."""
import math

import numpy as np
import pytest

import hp_policy
import hp_reference as hp
import joint_zoo
from fast_kinematic_simulator_amd import PolicyTable, _capi, policy_select
from fast_kinematic_simulator_amd import workloads as W
from fast_kinematic_simulator_amd.robots import rotation_from_axis_angle, se3_pose

U = 2.0 ** -53
NEAR = 1e-9  # the project's near-decision margin
SIZES = (1, 63, 64, 65, 200)
N_CONFIGS = 256
INDEX = 0x7FFFFFFF


def _robots():
    return {"cfg1": W.cfg1(1.0).robot, "cfg4": W.cfg4(1.0).robot, "cfg3": W.cfg3(1.0).robot,
            "folding_arm_continuous": W.folding_arm(0.5, continuous=True).robot, "mixed_tree": joint_zoo.mixed_tree().robot}


def _c(robot):
    if robot.robot_type == _capi.ROBOT_LINKED:
        return robot.config_width / 2.0 + 3.0
    if robot.robot_type == _capi.ROBOT_SE2:
        return 5.0
    return 5.5 + 44.0 * float(robot.distance_weights[1])


def _draw(robot, rng, count, beyond):
    """count configurations; `beyond`: some outside their joint limits, continuous dofs and the
    SE(2) angle up to three turns out"""
    if robot.robot_type == _capi.ROBOT_SE2:
        th = rng.uniform(-3 * np.pi, 3 * np.pi, count) if beyond else rng.uniform(-np.pi, np.pi, count)
        return np.column_stack([rng.uniform(0.2, 3.8, count), rng.uniform(0.2, 3.8, count), th])
    if robot.robot_type == _capi.ROBOT_SE3:
        out = []
        for _ in range(count):
            axis = rng.normal(size=3)
            out.append(se3_pose(rng.uniform(-1.0, 1.0, 3), rotation_from_axis_angle(axis / np.linalg.norm(axis), rng.uniform(-np.pi, np.pi))))
        return np.asarray(out, dtype=np.float64).reshape(count, 12)
    cols = []
    for continuous, lo, hi in hp_policy.dof_kinds(robot):
        if continuous:
            cols.append(rng.uniform(-3 * np.pi, 3 * np.pi, count) if beyond else rng.uniform(-np.pi, np.pi, count))
        else:
            span = hi - lo
            cols.append(rng.uniform(lo - 0.2 * span, hi + 0.2 * span, count) if beyond else rng.uniform(lo, hi, count))
    return np.column_stack(cols)


@pytest.fixture(scope="module")
def cases(fks_lib):
    """per robot: 256 configurations, a pool of 200 keys (a table of M entries is its first M) and
    the high-precision distances [256][200], computed once"""
    out = {}
    for seed, (name, robot) in enumerate(_robots().items()):
        rng = np.random.default_rng(100 + seed)
        configs = _draw(robot, rng, N_CONFIGS, beyond=True)
        keys = _draw(robot, rng, max(SIZES), beyond=False)
        targets = _draw(robot, rng, max(SIZES), beyond=False)
        out[name] = {"robot": robot, "configs": configs, "keys": keys, "targets": targets,
                     "hp": hp_policy.distances(robot, keys, configs)}
    return out


def test_the_test_inputs_leave_their_ranges(cases):
    """configurations outside their limits and continuous dofs beyond +-pi are in the draw"""
    for name, case in cases.items():
        robot, q = case["robot"], case["configs"]
        _, wrapped = hp_policy.reset_position(robot, q)
        if robot.robot_type == _capi.ROBOT_SE2 or any(k[0] for k in hp_policy.dof_kinds(robot) if robot.robot_type == _capi.ROBOT_LINKED):
            assert wrapped.any(), name
        if robot.robot_type == _capi.ROBOT_LINKED:
            kinds = hp_policy.dof_kinds(robot)
            outside = [np.any((q[:, k] < lo) | (q[:, k] > hi)) for k, (cont, lo, hi) in enumerate(kinds) if not cont]
            assert all(outside), name


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name", ["cfg1", "cfg4", "cfg3", "folding_arm_continuous", "mixed_tree"])
def test_selection_and_distance_against_high_precision(cases, name, M):
    case = cases[name]
    robot = case["robot"]
    table = PolicyTable(case["keys"][:M], case["targets"][:M])
    got = policy_select(robot, table, case["configs"])
    d = case["hp"]["d"][:, :M]
    rows = np.arange(N_CONFIGS)
    assert np.all(got["choice"] < M)  # no terminal entry, never lost: plain indices
    chosen = got["choice"].astype(np.int64)
    d_min = d.min(axis=1)
    # the reference's own near decisions: two entries within the margin of the minimum
    near = np.array([(d[c] <= d_min[c] * (1 + hp.DEFAULT.scalar(NEAR))).sum() > 1 for c in rows])
    assert near.mean() <= 0.03
    assert np.all(d[rows, chosen] <= d_min * (1 + hp.DEFAULT.scalar(NEAR)))
    # out_distance: the derived bound
    d_chosen = d[rows, chosen]
    skip = case["hp"]["near_pi"][:, :M][rows, chosen]
    assert skip.mean() <= 0.03
    err = np.array([abs(float(hp.DEFAULT.scalar(got["distance"][c]) - d_chosen[c])) for c in rows])
    d64 = hp.to_float(d_chosen)
    bound = (_c(robot) * U * np.maximum(1.0, d64) + 4 * U * math.pi * case["hp"]["wraps"][:, :M][rows, chosen]) * (1 + 2.0 ** -40)
    ratio = (err / bound)[~skip]
    print(f"policy_select {name} M={M}: worst |error| / bound = {ratio.max():.3f}, near {near.sum()}, near pi {skip.sum()}")
    assert np.all(ratio <= 1.0), (name, M, float(ratio.max()))


def test_both_backends_state_the_same_distances(cases):
    """the long-double statement against mpmath at 40 digits, on a corner of every robot's case"""
    other = hp.Backend("mpmath" if hp.DEFAULT.kind == "longdouble" else "longdouble")
    if other.kind == "longdouble" and np.finfo(np.longdouble).eps >= 1e-18:
        return  # one backend on this platform
    for name, case in cases.items():
        a = hp_policy.distances(case["robot"], case["keys"][:5], case["configs"][:8])
        b = hp_policy.distances(case["robot"], case["keys"][:5], case["configs"][:8], other)
        for x, y in zip(np.asarray(a["d"]).reshape(-1), np.asarray(b["d"]).reshape(-1)):
            assert abs(float(x) - float(y)) <= 8 * 2.0 ** -63 * max(1.0, float(y)) + 1e-17, name
        assert np.array_equal(a["wraps"], b["wraps"]) and np.array_equal(a["near_pi"], b["near_pi"])


# ---- the exact rules, compared with ==
def _se2():
    return W.cfg1(1.0).robot


def test_a_duplicate_at_a_higher_index_is_never_chosen(cases):
    for name, case in cases.items():
        keys = np.concatenate([case["keys"][:40], case["keys"][:40]])
        got = policy_select(case["robot"], PolicyTable(keys, keys), case["configs"])
        assert np.all(got["choice"] < 40), name
        first = policy_select(case["robot"], PolicyTable(keys[:40], keys[:40]), case["configs"])
        assert np.array_equal(got["choice"], first["choice"]) and np.array_equal(got["distance"], first["distance"])


def test_a_table_of_nan_keys_is_lost(cases):
    for name, case in cases.items():
        keys = np.full((5, case["robot"].config_width), np.nan)
        got = policy_select(case["robot"], PolicyTable(keys, case["targets"][:5], terminal=np.ones(5, bool), terminal_distance=np.inf),
                            case["configs"][:16])
        assert np.all(got["choice"] == _capi.POLICY_LOST), name
        assert np.all(got["distance"] == np.inf), name


def test_terminal_and_lost_are_strict_and_lost_comes_first():
    robot = _se2()
    q = np.array([[1.0, 1.0, 0.25]])
    keys = np.array([[1.5, 1.25, 0.5], [3.0, 3.0, 0.0]])
    terminal = np.array([True, False])
    d = policy_select(robot, PolicyTable(keys, keys), q)["distance"][0]
    assert 0.0 < d < np.inf

    def verdict(terminal_distance, max_distance):
        r = policy_select(robot, PolicyTable(keys, keys, terminal, terminal_distance, max_distance), q)
        assert r["distance"][0] == d
        return int(r["choice"][0])

    assert verdict(d, np.inf) == 0                                       # d == terminal_distance: not arrived
    assert verdict(np.nextafter(d, np.inf), np.inf) == _capi.POLICY_ARRIVED  # entry 0, arrived
    assert verdict(0.0, d) == 0                                          # d == max_distance: not lost
    assert verdict(0.0, np.nextafter(d, 0.0)) == _capi.POLICY_LOST
    assert verdict(np.inf, np.nextafter(d, 0.0)) == _capi.POLICY_LOST    # the lost test wins over the terminal test
    # a non-terminal entry never arrives
    r = policy_select(robot, PolicyTable(keys[::-1].copy(), keys, terminal, np.inf, np.inf), q)
    assert int(r["choice"][0]) == 1


def test_the_selection_is_of_the_reset_position():
    """a joint value beyond its limit is clamped before the distances are taken: the nearest key of
    the clamped value, not of the raw one"""
    robot = W.folding_arm(0.5, continuous=True).robot  # limits +-3 on dofs 1 and 2, dof 0 continuous
    q = np.array([[0.0, 4.0, 0.0]])
    keys = np.array([[0.0, 2.9, 0.0], [0.0, 4.0, 0.0]])
    r = policy_select(robot, PolicyTable(keys, keys), q)
    assert int(r["choice"][0]) == 0 and r["distance"][0] == 3.0 - 2.9
    # and a continuous dof three turns out is its representative in (-pi, pi]
    q = np.array([[0.5 + 6 * np.pi, 0.0, 0.0]])
    keys = np.array([[3.0, 0.0, 0.0], [0.4, 0.0, 0.0]])
    assert int(policy_select(robot, PolicyTable(keys, keys), q)["choice"][0]) == 1


def test_the_wrap_is_inside_the_distance():
    robot = _se2()
    q = np.array([[1.0, 1.0, 3.0]])
    keys = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, -3.0]])  # across the seam -3 is 0.28 away, 1.0 is 2.0 away
    r = policy_select(robot, PolicyTable(keys, keys), q)
    assert int(r["choice"][0]) == 1
    assert abs(r["distance"][0] - float(robot.distance_weights[1]) * (2 * np.pi - 6.0)) < 1e-14


# ---- refusals that need no device
def test_policy_select_refuses_malformed_arguments(fks_lib):
    robot = _se2()
    q = np.zeros((1, 3))
    keys = np.zeros((2, 3))
    with pytest.raises(_capi.FksError):
        policy_select(robot, PolicyTable(np.zeros((0, 3)), np.zeros((0, 3))), q)
    with pytest.raises(_capi.FksError):
        policy_select(robot, PolicyTable(keys, keys, terminal_distance=float("nan")), q)
    with pytest.raises(_capi.FksError):
        policy_select(robot, PolicyTable(keys, keys, max_distance=float("nan")), q)
    assert fks_lib.fks_policy_select(None, None, None, 0, None, None) == 1


def test_policy_entries_refuse_a_null_context(fks_lib):
    assert fks_lib.fks_forward_simulate_policy(None, None, 0, None, 1, 1, None, None, None, None, None, None, None, None) == 1
    assert fks_lib.fks_forward_simulate_policy_device(None, None, 0, None, 1, 0, 1, None, None, None, None, None, None, None, None,
                                                      None, 1) == 1


def test_kernel_kinds_name_the_policy_kernels():
    assert _capi.KERNEL_KINDS[16] == "policy" and _capi.KERNEL_KINDS[17] == "policy_small_batch"
