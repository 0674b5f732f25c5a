"""Replay of traced resolver iterations against tests/hp_contact.py: the scenes, the per-iteration
bound and the checks shared by tests/test_contact_replay_cpu.py (the oracle) and
tests/test_contact_replay.py (the HIP kernels).  Test helper, not a test module.

A traced run records the configuration before and after every resolver iteration.  One iteration
is a smooth map of its input away from its discrete decisions, so each recorded iterate is
recomputed from its predecessor in high precision and compared with the record.

The bound on |recorded - reference| per element of the next configuration:

    2^-53 . c . kappa_2(J_S) . max(|dq|_inf, F)

J_S the pivot columns of the solve, dq the applied step, F = 16 (n + 1) max(1, reach) the forward-
kinematics bound of DESIGN.md §3 for the deepest corrected link *in units of 2^-53* (taken with its
own 2^-53 the product would be quadratic in the unit roundoff).  The two arguments of the max are
the two ways an error reaches the step: relative to the step (the arithmetic of the solve and of
the scaling) and absolute (J and b carry the kinematics' error F 2^-53, which the solve turns into
an error of the step of kappa times as much; the final sum q + dq rounds at 2^-53 |q| <= 2^-53 F).

c counts the rounded operations an element can pass through, worst case, each counted once and
linearly (R rows, D columns):

    D (2 R + 3)   D Householder reflections, each a dot product of <= R products and R sums, then
                  one product with tau, one with v and one subtraction (Q' b is one more column)
    2 D + 1       back substitution: <= D products and differences and one division
    21            b's own arithmetic: the cell centre (3), p - centre (1), the gradient's division
                  (2), its dot product (5), the nominal value's shift and the sum (2), the normal's
                  norm (6) and division (1), the product with the penetration (1)
    2             the perturbations of J and of b by the kinematics, one F each
    48            the step: two world points and their distance for the motion estimate (12), the
                  division by step_fraction, the scaling, q + dq (3), the wrap (4), or SE(3)'s
                  P exp(twist) (about 30)

    c(R, D) = 2 D R + 5 D + 72.

For the individual-Jacobian form the step is a sum of per-point solves: the bound is the sum of
their bounds (R = 3 each).

An iteration with a near decision (hp_contact's docstring) is not compared and counts as skipped,
with three exceptions that are compared first and count as skipped only if that comparison fails: a
near rank decision (at the structural rank), an extended self-collision key within 1e-9 of an
integer (at the key of the header's double arithmetic) and a near pivot tie that leads to other
pivot columns (at the pivot taken or at a rival).

J is held row block by row block to the Jacobian bound of DESIGN.md §3 (2^-53 F of the block's
point, SE(2) / SE(3) with n = 1), b to what follows from the definitions: |gradient|_1 times the
point's bound plus 21 roundings of max(|b|, res) for an environment correction, and for a
self-collision correction cond(A) L (4 p / dt + 8 p v / d + 64 2^-53 v), L links in the impulse
system, p the point bound, v the fastest link velocity, d the shortest contact-normal baseline, A
the impulse matrix (velocities are differences of two points over dt, normals differences of two
points over their distance)."""
import dataclasses
import time

import numpy as np

import hp_contact as C
import hp_reference as H
import joint_zoo as Z
from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd import workloads as W
from fast_kinematic_simulator_amd.trace import (TRACE_CONTACT_STOP, TRACE_POST_ACTION, TRACE_RESOLVE_FAILED,
                                                TRACE_RESOLVER_STEP)

U = 2.0 ** -53
MAX_REPLAYED = 128
MAX_FREE_CHECKED = 64
SKIP_CAP = 0.03
MOVED_FLOOR = 0.90
CONFIG_CAPACITY = 16384


def _resolver_params():
    wl = W.folding_arm(0.25)
    wl.solver = dataclasses.replace(wl.solver, resolve_correction_step_scaling_decay_rate=0.7,
                                    resolve_correction_initial_step_size=0.8, resolve_correction_min_step_scaling=0.1,
                                    resolve_correction_step_scaling_decay_iterations=3, max_resolver_iterations=15)
    return wl


def with_environment(wl, env):
    """the workload `wl` around the environment `env`: a new Workload whose builder returns it"""
    return W.Workload(wl.name, wl.description, wl.robot, lambda: env, wl.starts, wl.targets, wl.solver, wl.controller_frequency,
                      wl.seed, wl.allow_contacts, wl.grid_cells, wl.resolution)


def _tied_normals():
    """cfg1 in a copy of its environment where every cell's surface-normal entries are followed by a copy
    of themselves with the normal turned a quarter about z: each entry direction then occurs twice, with
    bit-equal dot products and different normals, and the strict > of SPCS:100 / 123 decides (the first
    wins, so the run is cfg1's)."""
    from fast_kinematic_simulator_amd.environment import SimulatorEnvironment

    wl = W.cfg1(8 / 32)
    env = wl.environment()
    offsets, entries = env.normal_offsets.astype(np.int64), env.normal_entries.reshape(-1, 6)
    counts = np.diff(offsets)
    cell = np.repeat(np.arange(len(counts)), counts)
    turned = entries.copy()
    turned[:, 3], turned[:, 4] = -entries[:, 4], entries[:, 3]
    order = np.argsort(np.concatenate([cell, cell]), kind="stable")  # per cell: its entries, then their copies
    doubled = np.concatenate([entries, turned], axis=0)[order]
    wl = with_environment(wl, SimulatorEnvironment(env.geometry, env.sdf, np.concatenate([[0], np.cumsum(2 * counts)]),
                                                   doubled.reshape(-1), env.oob_value, env.occupancy))
    wl.name = "tied_normals"
    return wl


# name -> (workload builder at its smallest size, individual Jacobians)
SCENES = {
    "cfg1": (lambda: W.cfg1(8 / 32), False),
    "cfg2": (lambda: W.cfg2(8 / 4096), False),
    "cfg3": (lambda: W.cfg3(4 / 65536), False),
    "cfg4": (lambda: W.cfg4(16 / 1048576), False),
    "cfg5": (lambda: W.cfg5(2 / 1048576), False),
    "folding_arm": (lambda: W.folding_arm(0.25), False),
    "telescope": (lambda: Z.telescope(8), False),
    "mixed_tree": (lambda: Z.mixed_tree(4), False),
    "gantry": (lambda: Z.gantry(4), False),
    "wide_mixed": (lambda: Z.wide_mixed(8), False),
    "resolver_params": (_resolver_params, False),
    "individual_jacobians": (lambda: W.cfg3(4 / 65536), True),
    "tied_normals": (_tied_normals, False),
}


_ENVIRONMENTS = {}


def scene(name, device=None):
    """(workload, individual Jacobians) of a scene; scenes with the same environment builder share one
    environment, built on the host or, with `device`, on that HIP device (the same bytes, and the 512^3
    grid of cfg5 takes a fraction of the host's 25 s there)"""
    build, individual = SCENES[name]
    wl = build()
    if name == "tied_normals":
        return wl, individual  # its environment is its own
    key = (wl.env_builder if wl.name not in W.SCENES else wl.name, device)
    if key not in _ENVIRONMENTS:
        env = W.SCENES[wl.name](device=device) if device is not None and wl.name in W.SCENES else wl.environment()
        if wl.name == "cfg5":  # used once, and more than a gigabyte
            return with_environment(wl, env), individual
        _ENVIRONMENTS[key] = env
    return with_environment(wl, _ENVIRONMENTS[key]), individual


def c_of(R, D):
    return 2 * D * R + 5 * D + 72


def kinematics_scale(robot, q, g, point):
    """F of the module docstring for a point of geometry g: the bound of DESIGN.md §3 in units of 2^-53"""
    p = float(np.linalg.norm(np.asarray(point, dtype=np.float64)[:3]))
    if robot.robot_type == _capi.ROBOT_SE2:
        return 32.0 * max(1.0, float(np.hypot(q[0], q[1])) + p)
    if robot.robot_type == _capi.ROBOT_SE3:
        return 32.0 * max(1.0, float(np.linalg.norm(np.asarray(q, dtype=np.float64)[[3, 7, 11]])) + p)
    link = robot.geometry_link[g]
    return 16.0 * (len(H.link_path(robot, link)) + 1) * max(1.0, H.reach(robot, link, point))


def iteration_bound(robot, active, result):
    F = max(kinematics_scale(robot, active, g, robot.geometry_points[g][i]) for g, i in result["corrected"])
    dq = float(np.max(np.abs(H.to_float(result["real_step"]))))
    D = robot.num_dofs
    return U * sum(c_of(R, D) * kappa for R, _, kappa in result["solves"]) * max(dq, F)


class Replay:
    """The records of one traced run, addressed the way the resolver loop produced them."""

    def __init__(self, wl, buf, reference):
        self.wl, self.buf, self.ref = wl, buf, reference
        self.n = len(wl.starts)
        assert np.all(buf.num_configs <= buf.config_capacity) and np.all(buf.num_steps <= buf.step_capacity), "trace truncated"
        self.start = [H.to_float(reference.set_position(wl.starts[i])) for i in range(self.n)]

    def tags(self, i):
        return self.buf.config_tags[i, :int(self.buf.num_configs[i])]

    def microstep_start(self, i, k):
        """index of the POST_ACTION record of record k's microstep"""
        kinds = self.tags(i)[:, 2]
        while kinds[k] != TRACE_POST_ACTION:
            k -= 1
        return k

    def previous(self, i, post):
        """the configuration the microstep whose POST_ACTION record is `post` started from"""
        return self.buf.configs[i, post - 1] if post > 0 else self.start[i]

    def records(self, kind):
        return [(i, k) for i in range(self.n) for k in np.nonzero(self.tags(i)[:, 2] == kind)[0]]

    def expected_in_collision(self, i, k):
        """what the trace shows about the collision check after record k (SPCS:1611-1625, 1694-1715).  The
        iteration limit (SPCS:1705) also ends a resolve whose last iterate happens to be free with a
        RESOLVE_FAILED record; no replayed record of the scenes is one, and it would show as a verdict
        mismatch to look at, not as a pass."""
        tags = self.tags(i)
        if k + 1 >= len(tags):
            return False
        nxt = int(tags[k + 1, 2])
        if nxt in (TRACE_RESOLVER_STEP, TRACE_RESOLVE_FAILED):
            return True
        if nxt == TRACE_CONTACT_STOP:
            assert int(tags[k, 2]) == TRACE_POST_ACTION
            return True
        return False


CELL_KEY = "self-collision cell"
PIVOT_TIE = "pivot choice"


def only_cell_keys_near(M):
    """every near decision is an extended-cell key within 1e-9 of an integer that matters"""
    return bool(M.near) and all(kind == CELL_KEY for kind, _ in M.near)


def with_double_keys(ref, evaluate):
    """`evaluate()` with the near extended keys taken in the header's double arithmetic (hp_contact._self_keys)"""
    ref.double_keys = True
    try:
        return evaluate()
    finally:
        ref.double_keys = False


def strided(items, limit):
    """at most `limit` items at a fixed stride over all of them"""
    stride = max(1, -(-len(items) // limit))
    return items[::stride][:limit]


def replay_scene(name, wl, buf, individual, systems=None, B=H.DEFAULT, limit=MAX_REPLAYED):
    """Replays a traced run (module docstring); returns the scene's figures.  `systems`: the (J, b)
    the run solved, in trace order (particle after particle), if they are to be compared."""
    t0 = time.time()
    robot = wl.robot
    ref = C.ContactReference(wl.environment(), robot, wl.solver, 1.0 / wl.controller_frequency, individual, B)
    rp = Replay(wl, buf, ref)
    steps = rp.records(TRACE_RESOLVER_STEP)
    order = {rec: n for n, rec in enumerate(steps)}
    chosen = strided(steps, limit)
    assert chosen, f"{name}: no resolver iteration in the trace"
    stats = {"replayed": 0, "skipped": 0, "near_keys": 0, "near_ties": 0, "tie_fallbacks": 0, "moved": 0, "compared": 0,
             "rank_fallbacks": 0, "worst": 0.0, "worst_relative": 0.0, "worst_J": 0.0, "worst_b": 0.0, "systems": 0, "self_corrected": 0, "max_abs": 0.0}
    failures, fallen = [], []  # fallen: near decisions whose first comparison failed (skipped, kept for the report)
    for i, k in chosen:
        post = rp.microstep_start(i, k)
        previous, active, record = rp.previous(i, post), buf.configs[i, k - 1], buf.configs[i, k]
        r = ref.iterate(previous, active, k - post - 1)
        stats["replayed"] += 1
        stats["moved"] += int(not np.array_equal(record, active))
        by_double_keys = only_cell_keys_near(r["margins"])
        if by_double_keys:
            stats["near_keys"] += 1
            r = with_double_keys(ref, lambda: ref.iterate(previous, active, k - post - 1))
        M = r["margins"]
        stats["self_corrected"] += r["self_corrected"]
        if any(kind != PIVOT_TIE for kind, _ in M.near):
            stats["skipped"] += 1
            continue
        assert r["next"] is not None, f"{name}: particle {i} record {k}: the reference finds nothing to correct"
        expected = rp.expected_in_collision(i, k)

        def measure(c):
            err = float(np.max(np.abs(H.to_float(c["next"] - B.array(record)))))
            return err, iteration_bound(robot, active, {**c, "corrected": r["corrected"]})

        err, bound = measure(r)
        verdict = r["in_collision"]
        tie = bool(M.near)
        if tie and (err > bound or verdict != expected):
            # unequal pivot candidates within 1e-9 that lead to other pivot columns: the recorded iterate
            # has to be the one of the pivot taken here or of one of the rivals
            stats["tie_fallbacks"] += 1
            for raw, solves in r["rivals"]:
                evaluate = lambda: ref.rival(previous, active, k - post - 1, raw, solves)  # noqa: E731
                c = with_double_keys(ref, evaluate) if by_double_keys else evaluate()
                e, b = measure(c)
                if not c["margins"].near and e <= b and c["in_collision"] == expected:
                    err, bound, verdict = e, b, c["in_collision"]
                    break
        if (M.near_rank or by_double_keys or tie) and (err > bound or verdict != expected):
            # a near rank decision is compared at the structural rank first, a near extended key at the
            # header's double arithmetic first, a near pivot tie at either pivot: skipped only if that
            # comparison fails
            stats["skipped"] += 1
            stats["rank_fallbacks"] += int(bool(M.near_rank))
            fallen.append((err / bound, f"particle {i} record {k}: |next - reference| = {err:.3e} (bound {bound:.3e}), in collision "
                                        f"{verdict} (the trace: {expected})"))
            continue
        stats["compared"] += 1
        stats["near_ties"] += int(tie)
        stats["worst"] = max(stats["worst"], err / bound)
        stats["max_abs"] = max(stats["max_abs"], err)
        # for the record only: the ratio to a bound without the absolute term, 2^-53 (c kappa |dq| + |q|)
        dq = float(np.max(np.abs(H.to_float(r["real_step"]))))
        relative = U * (sum(c_of(R, robot.num_dofs) * kappa for R, _, kappa in r["solves"]) * dq + float(np.max(np.abs(record))))
        stats["worst_relative"] = max(stats["worst_relative"], err / relative)
        if err > bound:
            failures.append(f"particle {i} record {k}: |next - reference| = {err:.3e} > bound {bound:.3e}")
        if verdict != expected:
            failures.append(f"particle {i} record {k}: in collision {verdict} but the trace continues with "
                            f"{'a resolver record' if expected else 'the next microstep'}")
        if systems is not None:
            Jo, bo = systems[order[(i, k)]]
            wj, wb = compare_system(ref, robot, active, r, Jo, bo, failures, f"particle {i} record {k}")
            stats["worst_J"], stats["worst_b"] = max(stats["worst_J"], wj), max(stats["worst_b"], wb)
            stats["systems"] += 1
    stats["free_checked"], stats["free_skipped"] = check_free_post_actions(rp, ref, failures)
    stats["steps_checked"], stats["steps_skipped"] = check_microstep_counts(rp, ref, failures)
    stats["skip_share"] = stats["skipped"] / stats["replayed"]
    stats["moved_share"] = stats["moved"] / stats["replayed"]
    stats["seconds"] = time.time() - t0
    print(f"{name}: replayed {stats['replayed']} of {len(steps)} iterations, skipped {100 * stats['skip_share']:.1f} % "
          f"({stats['rank_fallbacks']} noise pivots; {stats['near_keys']} at double-arithmetic keys, {stats['near_ties']} with a near "
          f"pivot tie of which {stats['tie_fallbacks']} at a rival pivot), moved {100 * stats['moved_share']:.1f} %, worst ratio to the bound "
          f"{stats['worst']:.2e} (to 2^-53 (c kappa |dq| + |q|): {stats['worst_relative']:.2f}; largest difference {stats['max_abs']:.2e}), J {stats['worst_J']:.3f}, b {stats['worst_b']:.3f} "
          f"over {stats['systems']} systems, {stats['self_corrected']} self corrections, {stats['free_checked']} free post-action "
          f"records ({stats['free_skipped']} near), {stats['steps_checked']} microstep counts ({stats['steps_skipped']} near), "
          f"{stats['seconds']:.1f} s")
    assert not failures, f"{name}: " + "; ".join(failures[:8]) + (f" (+{len(failures) - 8} more)" if len(failures) > 8 else "")
    worst_fallen = max(fallen, default=None)
    assert stats["skip_share"] <= SKIP_CAP, (
        f"{name}: {stats['skipped']} of {stats['replayed']} iterations skipped"
        + (f"; {len(fallen)} of them were compared and failed, the worst at {worst_fallen[0]:.3g} of its bound: {worst_fallen[1]}"
           if fallen else ""))
    for what, checked, skipped in (("free post-action records", stats["free_checked"], stats["free_skipped"]),
                                   ("microstep counts", stats["steps_checked"], stats["steps_skipped"])):
        assert checked > 0, f"{name}: no {what} checked"
        assert skipped <= SKIP_CAP * (checked + skipped), f"{name}: {skipped} of {checked + skipped} {what} near a decision"
    assert stats["moved_share"] >= MOVED_FLOOR, f"{name}: only {stats['moved']} of {stats['replayed']} iterations moved"
    assert stats["worst"] <= 1.0
    return stats


def compare_system(ref, robot, active, r, Jo, bo, failures, where):
    """The recorded stacked system against the reference's, row for row."""
    J, b = H.to_float(r["J"]), H.to_float(r["b"])
    if Jo.shape != J.shape:
        failures.append(f"{where}: the solved system has {Jo.shape[0]} rows, the reference {J.shape[0]}")
        return np.inf, np.inf
    worst_J = worst_b = 0.0
    B, G = ref.B, ref.grid
    res, dt = G.res_f, float(ref.dt)
    for n, (g, i) in enumerate(r["corrected"]):
        rows = slice(3 * n, 3 * n + 3)
        tol = U * kinematics_scale(robot, active, g, robot.geometry_points[g][i])
        dJ = H.max_abs_diff(r["J"][rows], Jo[rows], B)
        db = H.max_abs_diff(r["b"][rows], bo[rows], B)
        # the gradient's 1-norm is at most 3 up to the floats' rounding: three central differences of a distance field
        tol_b = 3.0 * tol + 21 * U * max(float(np.max(np.abs(b[rows]))), res)
        if (g, i) in r["self_info"]:
            v, d, cond, links = r["self_info"][(g, i)]
            tol_b += cond * links * (4 * tol / dt + 8 * tol * v / max(d, 1e-300) + 64 * U * v)
        worst_J, worst_b = max(worst_J, dJ / tol), max(worst_b, db / tol_b)
        if dJ > tol:
            failures.append(f"{where}: Jacobian block of point ({g}, {i}) off by {dJ:.3e} > {tol:.3e}")
        if db > tol_b:
            failures.append(f"{where}: correction of point ({g}, {i}) off by {db:.3e} > {tol_b:.3e}")
    return worst_J, worst_b


def check_free_post_actions(rp, ref, failures):
    """POST_ACTION records the resolver did not run after: the reference must find them free."""
    free = [(i, k) for i, k in rp.records(TRACE_POST_ACTION) if not rp.expected_in_collision(i, k)]
    checked = skipped = 0
    for i, k in strided(free, MAX_FREE_CHECKED):
        def check():
            M = C.Margins()
            verdict, _ = ref.in_collision(ref.state(rp.previous(i, k)), ref.state(rp.buf.configs[i, k]), M)
            return {"verdict": verdict, "margins": M}

        r = check()
        by_double_keys = only_cell_keys_near(r["margins"])
        if by_double_keys:
            r = with_double_keys(ref, check)
        verdict = r["verdict"]
        if r["margins"].near or (by_double_keys and verdict):
            skipped += 1
            continue
        checked += 1
        if verdict:
            failures.append(f"particle {i} record {k}: a post-action configuration the trace treats as free is in collision")
    return checked, skipped


def check_microstep_counts(rp, ref, failures):
    """SPCS:1559-1562 for every controller step of every particle."""
    checked = skipped = 0
    buf = rp.buf
    for i in range(rp.n):
        tags = rp.tags(i)
        for s in range(int(buf.num_steps[i])):
            first = np.nonzero(tags[:, 0] == s)[0]
            if not len(first):
                continue
            q = buf.configs[i, first[0] - 1] if first[0] > 0 else rp.start[i]
            count, M = ref.microsteps(q, buf.step_inputs[i, s, 0])
            if M.near:
                skipped += 1
                continue
            checked += 1
            if count != int(buf.step_microsteps[i, s]):
                failures.append(f"particle {i} step {s}: {int(buf.step_microsteps[i, s])} microsteps, the reference {count}")
    return checked, skipped


# ---------------------------------------------------------------- CheckConfigCollision
CHECK_CONFIGS = 256
CHECK_INFLATIONS = (0.0, 0.5)
CHECK_SCENES = ("cfg3", "mixed_tree", "telescope")  # environment contact, the same on a tree, self contact
CHECK_RAYS, CHECK_SCAN, CHECK_BISECTIONS = 12, 16, 20
FLIP_FLOOR = 0.10

_CHECK_WORKLOADS = {}
_CHECK_REFERENCE = {}


def _reference_check(ref, q, inflation):
    """(verdict, Margins) of the reference; a configuration whose only near decisions are extended-cell keys
    is decided at the header's double arithmetic (hp_contact._self_keys)"""
    v, M = ref.check_config_collision(q, inflation)
    if only_cell_keys_near(M):
        v, M = with_double_keys(ref, lambda: ref.check_config_collision(q, inflation))
    return v, M


def _threshold_window(ref, at, t_contact, count):
    """Where the environment threshold of inflation 0.5 decides differently from that of inflation 0.
    Stored distances are multiples of the cell size (+-res next to a surface), so both thresholds
    (inflation res - tolerance res) fall between the same two stored values and the verdicts differ
    only through the estimate: a point in a cell of distance -res is a hit at inflation 0.5 whatever its
    estimate (its value is a whole cell below the threshold), and at inflation 0 only if its estimate
    is below -tolerance res = -1e-5 res.  The estimate starts above 0 where the point enters the cell
    (replaced by -res/16: a hit) and falls as it goes deeper; while it lies in (-tolerance res, 0) the
    configuration is free at inflation 0 and collides at 0.5.  That window is a few micrometres wide.
    From the first contact at t_contact the ray is walked in steps of 1e-4 until the shallowest
    penetrating point's estimate (hp_contact.shallowest_penetration) has fallen through the window,
    the estimates 0.1 and 0.9 of the way through it are found by bisection, and `count` parameters are
    returned: count - 2 across the window, the step behind it and one further."""
    tolerance = float(ref.solver.environment_collision_check_tolerance) * ref.grid.res_f
    step, a, b = 1e-4, t_contact, None
    for n in range(1, 120):
        h = ref.shallowest_penetration(at(t_contact + n * step))
        if h > 0.0:
            a = t_contact + n * step
        elif h < -tolerance:
            b = t_contact + n * step
            break
    if b is None or b - a > 1.5 * step:
        return [t_contact + n * step for n in range(1, count + 1)]  # another point came first: plain samples

    def where(level):
        lo_t, hi_t = a, b
        for _ in range(40):
            m = 0.5 * (lo_t + hi_t)
            lo_t, hi_t = (m, hi_t) if ref.shallowest_penetration(at(m)) > level else (lo_t, m)
        return 0.5 * (lo_t + hi_t)

    return list(np.linspace(where(-0.1 * tolerance), where(-0.9 * tolerance), count - 2)) + [b, b + step]


def check_workload(name):
    """(workload, 256 seeded configurations).  Half lie along and around the line from the first start
    through the target, where the simulation meets the obstacles or the robot itself, to 1.6 times as far.
    The other half are placed where the inflation ratio decides: on 12 rays from the start through a
    point around the target, the first contact at inflation 0.5 and at inflation 0 is bracketed by
    bisection on the reference's verdict (20 halvings of one scan step: about 1e-7 of the ray, far above
    a near decision).  For the telescope (self contact: the cell size (inflation + 1) res decides) the ray
    contributes the two brackets and points spread between them; for the others the bracket of inflation
    0.5 and the window of _threshold_window.  These are the configurations a check that ignored the
    inflation ratio would decide wrongly."""
    if name in _CHECK_WORKLOADS:
        return _CHECK_WORKLOADS[name]
    wl, _ = scene(name)
    ref = C.ContactReference(wl.environment(), wl.robot, wl.solver, 1.0 / wl.controller_frequency)
    lo, hi = wl.robot.dof_limits()
    rng = np.random.default_rng(61)
    start, line = wl.starts[0], wl.targets[0] - wl.starts[0]
    half = CHECK_CONFIGS // 2
    along = np.linspace(0.0, 1.6, half)[:, None]
    configs = [np.clip(start + along * line + rng.uniform(-0.25, 0.25, size=(half, len(lo))) * along, lo, hi)]
    per_ray = (CHECK_CONFIGS - half) // CHECK_RAYS
    placed = []
    for _ in range(CHECK_RAYS):
        direction = line + rng.uniform(-0.25, 0.25, size=len(lo))

        def at(t):
            return np.clip(start + t * direction, lo, hi)

        def first_contact(inflation, t_free):
            """(t free, t colliding) around the first contact past t_free, or None"""
            scan = np.linspace(t_free, 1.6, CHECK_SCAN)
            hit = next((t for t in scan[1:] if _reference_check(ref, at(t), inflation)[0]), None)
            if hit is None:
                return None
            a, b = scan[list(scan).index(hit) - 1], hit
            for _ in range(CHECK_BISECTIONS):
                m = 0.5 * (a + b)
                a, b = (a, m) if _reference_check(ref, at(m), inflation)[0] else (m, b)
            return a, b

        inflated = first_contact(CHECK_INFLATIONS[1], 0.0)
        if inflated is None:
            continue
        if name == "telescope":
            plain = first_contact(CHECK_INFLATIONS[0], inflated[0]) or (1.6, 1.6)
            ts = [inflated[0], inflated[1], plain[0], plain[1]]
            ts += list(np.linspace(inflated[1], plain[0], per_ray - 4 + 2)[1:-1])
        else:
            ts = [inflated[0], inflated[1]] + _threshold_window(ref, at, inflated[1], per_ray - 2)
        placed += [at(t) for t in ts]
    filler = CHECK_CONFIGS - half - len(placed)
    if filler:
        t = rng.uniform(0.0, 1.6, size=(filler, 1))
        placed += list(np.clip(start + t * line, lo, hi))
    configs = np.ascontiguousarray(np.concatenate([configs[0], np.array(placed)], axis=0))
    assert configs.shape[0] == CHECK_CONFIGS
    configs.flags.writeable = False
    _CHECK_WORKLOADS[name] = (wl, configs)
    return _CHECK_WORKLOADS[name]


def check_reference(name, inflation):
    """(verdicts, near flags, environment verdicts, self verdicts) of the reference's CheckConfigCollision,
    computed once per (scene, inflation)"""
    key = (name, float(inflation))
    if key not in _CHECK_REFERENCE:
        wl, configs = check_workload(name)
        ref = C.ContactReference(wl.environment(), wl.robot, wl.solver, 1.0 / wl.controller_frequency)
        out = np.zeros((4, len(configs)), dtype=bool)
        for n, q in enumerate(configs):
            v, M = _reference_check(ref, q, inflation)
            out[:, n] = v, bool(M.near), M.parts[0], M.parts[1]
        out.flags.writeable = False
        _CHECK_REFERENCE[key] = tuple(out)
    return _CHECK_REFERENCE[key]


def check_flip_shares(name):
    """shares of the configurations whose reference verdict differs between the two inflation ratios:
    (the whole verdict, the environment check's, the self check's); near configurations do not count"""
    a, b = (check_reference(name, inflation) for inflation in CHECK_INFLATIONS)
    clear = ~a[1] & ~b[1]
    return tuple(float(np.mean((a[k] != b[k]) & clear)) for k in (0, 2, 3))


def compare_config_checks(name, collided_by_inflation):
    """the collided flags of the CheckConfigCollision batches (one per inflation ratio) against the
    reference's verdicts.  The configurations are worth the second ratio only if it changes verdicts:
    at least 10 % of them must flip, through the environment threshold inflation res (cfg3,
    mixed_tree) or through the self check's cell size (inflation + 1) res (telescope)."""
    whole, through_env, through_self = check_flip_shares(name)
    print(f"{name}: verdict flips between inflation {CHECK_INFLATIONS[0]} and {CHECK_INFLATIONS[1]}: {100 * whole:.1f} % "
          f"(environment check {100 * through_env:.1f} %, self check {100 * through_self:.1f} %)")
    assert whole >= FLIP_FLOOR, f"{name}: only {100 * whole:.1f} % of the configurations depend on the inflation ratio"
    assert (through_self if name == "telescope" else through_env) >= FLIP_FLOOR, (name, through_env, through_self)
    for inflation, collided in zip(CHECK_INFLATIONS, collided_by_inflation):
        verdicts, near = check_reference(name, inflation)[:2]
        share = float(np.mean(near))
        colliding, free = float(np.mean(verdicts[~near])), float(np.mean(~verdicts[~near]))
        wrong = np.nonzero((np.asarray(collided, dtype=bool) != verdicts) & ~near)[0]
        print(f"{name} inflation {inflation}: {100 * colliding:.1f} % collide, {100 * free:.1f} % free, {100 * share:.1f} % near")
        assert share <= SKIP_CAP, f"{name}: {int(near.sum())} of {len(near)} configurations near a decision"
        assert colliding >= 0.10 and free >= 0.10, (colliding, free)
        assert not len(wrong), f"{name} inflation {inflation}: configurations {wrong[:8]} decided differently"
