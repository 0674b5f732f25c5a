"""Replay of the actuation half of traced runs against tests/hp_actuation.py: the scenes, the bounds and the
checks shared by tests/test_actuation_replay_cpu.py (the oracle, the host twins) and
tests/test_actuation_replay.py (the HIP kernels).  Test helper, not a test module.

From a traced run, for every recorded controller step and microstep:

 (a) the step's control_input (clamp(term, +-vmax) dt, SPCS:1549) against the reference controller, fed the
     configuration the trace holds at the step's start and carrying its own PID state from zero (or from the
     state a mutable-robot call passes in);
 (b) control_input_step = control_input / number_microsteps (SPCS:1568, from the recorded input and count:
     one division, U of the quotient), and the count's use: the step's post-action records carry the
     microsteps 0, 1, ... in order and all number_microsteps of them unless the step ends with a failed
     resolve or a contact stop;
 (c) every post-action record against the noisy application of control_input_step to the configuration that
     microstep started from (the previous microstep's last record, or the step's start).  A post-action
     record precedes any resolver work, so every microstep is comparable, in contact or free.

The bounds per element are counted operation by operation in hp_actuation (truncated_normal, twist_bound,
controller_step, applied_input, noisy_apply): the draw 2^-53 . 5 . |n| (1 + 1 / |ln r2|); a linked or SE(2)
element the draw's bound times the noise bound plus the roundings of the products and of the two sums
(4 2^-53 pi more for a wrapped element, compared modulo 2 pi); SE(3) the P exp(twist) bound of DESIGN §3 plus
(1 + |v|) times the 2-norm of the twist's noise error; the SE(3) error twist 2^-53 c max(1, |t|) (1 + 1 / s), c = 270
for the translation part and 54 for the rotation part, without 1 / s but with the branch's truncation 2 s^2
at pi, with the series' remainder below 1e-3.

A decision within 1e-9 relative of its threshold (r2 against 1, a candidate against +-2, the PID integral
against its clamp, the term against +-vmax, the clamped input against a sampled bin's edge) is not compared
and counts as skipped: at most 1 % of a scene's microsteps and none of its controller steps' inputs.

A scene is asserted to reach what it is there for (Scene's flags): PID terms inside the velocity clamp (where the
term is clamped, control_input shows only sign vmax dt), steps that outrun the noise buffer, joint limits,
wraps, both arms of the noise bound, a passed-in PID state that changes control_input beyond its bound."""
import dataclasses
import time

import numpy as np

import contact_replay as R
import hp_actuation as A
import hp_reference as H
import joint_zoo as Z
from fast_kinematic_simulator_amd import _capi
from fast_kinematic_simulator_amd import workloads as W
from fast_kinematic_simulator_amd.trace import TRACE_CONTACT_STOP, TRACE_POST_ACTION, TRACE_RESOLVE_FAILED

U = A.U
SKIP_CAP = 0.01
CONFIG_CAPACITY = 2048
NOISE_SLOTS = 64  # the kernels draw the noise of floor(64 / D) microsteps at a time


@dataclasses.dataclass
class Scene:
    name: str
    wl: object
    call_index: int = 0
    first_particle_id: int = 0
    controller_state: object = None  # (n, 2 D): a mutable-robot call
    individual: bool = False
    either_sign: tuple = ()          # particles whose relative rotation is pi exactly: the axis up to its sign
    both_arms: bool = False          # both arms of the noise bound's max must decide
    limits: bool = False             # a post-action value must sit on a joint limit
    wraps: bool = False              # a post-action value must have been wrapped
    controller: bool = True          # some dof's PID term must stay inside the velocity clamp in some step
    refill: object = None            # a step must outrun the noise buffer (None: linked robots only)


def _sized(wl, n, steps, env_of=None, device=None, vmax=None, kp=None):
    """`wl` cut to n particles and `steps` controller steps, in the (cached) environment of contact_replay's
    scene `env_of`; vmax: the velocity limit of every dof, raised so that a step has more microsteps than
    the noise buffer holds; kp: the proportional gain of every dof, raised so that the term reaches that limit"""
    if env_of is not None:
        wl = R.with_environment(wl, R.scene(env_of, device)[0].environment())
    wl.starts = np.ascontiguousarray(wl.starts[:n])
    if len(wl.targets) > 1:
        wl.targets = np.ascontiguousarray(wl.targets[:n])
    wl.solver = dataclasses.replace(wl.solver, forward_simulation_time=(steps + 0.5) / wl.controller_frequency)
    if vmax is not None:
        wl.robot = dataclasses.replace(wl.robot, controllers=[dataclasses.replace(c, velocity_limit=vmax, acceleration_limit=10 * vmax)
                                                              for c in wl.robot.controllers])
    if kp is not None:
        wl.robot = dataclasses.replace(wl.robot, controllers=[dataclasses.replace(c, kp=kp) for c in wl.robot.controllers])
    return wl


def _cfg3(device, n=4, steps=4):
    """cfg3 with the targets of the four wrist-side dofs moved to within 0.02 to 0.11 of the nominal start: their
    PID terms stay inside the velocity clamp (kp = 10, vmax = 1.5), so the error, the integral, the derivative
    and the gains show in control_input; the three base dofs keep their far targets and with them a step's
    microstep count above the noise buffer's"""
    wl = _sized(W.cfg3(n / 65536), n, steps, "cfg3", device, vmax=1.5)
    wl.targets = wl.targets.copy()
    wl.targets[:, 3:] = W.CFG3_NOMINAL[3:] + np.array([0.11, -0.06, 0.02, -0.09])
    return wl


def _sampled(device):
    from test_sampled_actuator import _with_sampled

    wl = _cfg3(device)
    wl.robot = _with_sampled(wl)
    return Scene("sampled", wl)


def _noise_floor(device):
    """a small proportional bound and a non-zero minimum.  A dof at its velocity limit has |real| = vmax dt /
    (microsteps of the step), some 8e-4 vmax, so prop |real| = 4e-5 vmax lies above the minimum of the even dofs
    (1e-5 vmax) and below that of the odd ones (1e-3 vmax); a dof close to its target has a smaller |real|"""
    wl = _cfg3(device)
    wl.robot = dataclasses.replace(wl.robot, controllers=[dataclasses.replace(c, max_actuator_proportional_noise=0.05,
                                                                               max_actuator_minimum_noise=1e-3 if k % 2 else 1e-5)
                                                          for k, c in enumerate(wl.robot.controllers)])
    return Scene("noise_floor", wl, both_arms=True)


def _mixed_tree(device):
    """the prismatic dof 4 starts 0.05 above its lower limit and is sent past it (the branch's last link moves
    away from the others); dof 2 is continuous and is sent the short way round through pi"""
    wl = _sized(Z.mixed_tree(4), 4, 5, "mixed_tree", device, vmax=2.5)
    wl.targets = wl.targets.copy()
    wl.targets[:, 4] = -0.3
    return Scene("mixed_tree", wl, limits=True, wraps=True)


def _telescope(device):
    """the prismatic dof starts 0.05 above its lower limit and is sent past it"""
    wl = _sized(Z.telescope(4), 4, 5, "telescope", device, vmax=4.0)
    wl.starts[:, 1] -= 0.25
    wl.targets = wl.targets.copy()
    wl.targets[:, 1] = -0.4
    return Scene("telescope", wl, limits=True)


def _mutable(device):
    """a mutable-robot call: a non-zero PID state per particle.  replay_scene asserts that the state shows: the
    reference's control_input from it and from a zeroed controller differ by more than their bounds"""
    wl = _cfg3(device)
    rng = np.random.default_rng(71)
    D = wl.robot.num_dofs
    state = np.concatenate([rng.uniform(-0.4, 0.4, size=(len(wl.starts), D)), rng.uniform(-0.05, 0.05, size=(len(wl.starts), D))], axis=1)
    return Scene("mutable", wl, controller_state=np.ascontiguousarray(state))


SE3_AXES = [(-0.8, 0.3, 0.5), (0.1, -0.9, 0.2), (0.8, 0.3, 0.5)]
SE3_DELTAS = (1e-2, 1e-4, 2e-6, 5e-7, 1e-7, 1e-9, 0.0)
# 9.99e-4 and 1.001e-3 straddle the series' threshold; 5e-3 and 9.9e-3 are where a series kept beyond it shows
SE3_THETAS = (0.0, 1e-9, 9.99e-4, 1.001e-3, 5e-3, 9.9e-3, 1.0, "pi/2", 3.0)
SE3_TRANSLATION = (0.3, -0.2, 0.5)


def se3_angle_cases(B=H.DEFAULT):
    """[(label, axis, relative transform 4x4 rounded to float64, whether both signs of the axis are right)]:
    every angle about the three axes and their negatives, translation (0.3, -0.2, 0.5)"""
    cases = []
    for base in SE3_AXES:
        for sign in (1.0, -1.0):
            axis = tuple(sign * a for a in base)
            angles = [(f"theta={t}", B.pi / 2 if t == "pi/2" else B.scalar(t), False) for t in SE3_THETAS]
            angles += [(f"pi-{d}", B.pi - B.scalar(d), d == 0.0) for d in SE3_DELTAS]
            for label, theta, either in angles:
                T = H.homogeneous(R=H.rodrigues(axis, theta, B), t=B.array(SE3_TRANSLATION), B=B)
                cases.append((f"{axis} {label}", axis, H.to_float(T), either))
    return cases


def _se3_angles(device):
    """cfg4's robot and environment, one controller step; particle i starts at a pose P_i near the origin and
    is sent to P_i Rel_i, Rel_i the i-th case of se3_angle_cases"""
    cases = se3_angle_cases()
    wl = _sized(W.cfg4(len(cases) / 1048576), len(cases), 1, "cfg4", device)
    targets = np.zeros((len(cases), 12))
    for i, (_, _, rel, _) in enumerate(cases):
        targets[i] = H.to_float((H.from34(wl.starts[i]) @ H.DEFAULT.array(rel))[:3, :]).reshape(12)
    wl.targets = targets
    return Scene("se3_angles", wl, either_sign=tuple(i for i, c in enumerate(cases) if c[3]))


SCENES = {
    # SE(2) and SE(3) read the same noise buffer (21 and 10 microsteps): velocity limits raised past it
    "cfg1": lambda device: Scene("cfg1", _sized(W.cfg1(8 / 32), 8, 5, "cfg1", device, vmax=10.0, kp=10.0), refill=True),
    "cfg3": lambda device: Scene("cfg3", _cfg3(device)),
    "cfg4": lambda device: Scene("cfg4", _sized(W.cfg4(8 / 1048576), 8, 4, "cfg4", device, vmax=1.5), refill=True),
    "cfg5": lambda device: Scene("cfg5", _sized(W.cfg5(4 / 1048576), 4, 3, "cfg5", device, vmax=1.5)),
    "mixed_tree": _mixed_tree,
    "telescope": _telescope,
    # every dof of the giant chain runs at its velocity limit: it is here for the buffer of one microstep
    "giant_chain": lambda device: Scene("giant_chain", _sized(W.giant_chain(1.0), 4, 3), controller=False),
    "sampled": _sampled,
    "noise_floor": _noise_floor,
    "call_index": lambda device: Scene("call_index", _cfg3(device), call_index=3),
    "individual_jacobians": lambda device: Scene("individual_jacobians", _cfg3(device), individual=True),
    "se3_angles": _se3_angles,
}
# the oracle's traced entry takes a first particle id and no controller state; the library's takes a
# controller state and no first particle id
CPU_ONLY = {"high_particle_id": lambda device: Scene("high_particle_id", _cfg3(device), call_index=2, first_particle_id=(5 << 32) + 7)}
GPU_ONLY = {"mutable": _mutable}


def scene(name, device=None):
    return {**SCENES, **CPU_ONLY, **GPU_ONLY}[name](device)


def oracle_traced(sc):
    import oracle

    wl = sc.wl
    res, buf = oracle.forward_simulate_traced(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, wl.starts,
                                              wl.targets, True, call_index=sc.call_index, config_capacity=CONFIG_CAPACITY, threads=1,
                                              first_particle_id=sc.first_particle_id, individual_jacobians=sc.individual)
    assert not np.any(res["error_flags"]), np.unique(res["error_flags"])
    return buf


def gpu_traced(sc):
    from fast_kinematic_simulator_amd import make_linked_simulator

    wl = sc.wl
    assert sc.first_particle_id == 0
    sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
    try:
        sim.set_individual_jacobians(sc.individual)
        sim.set_call_index(sc.call_index)
        if sc.controller_state is None:
            res, buf = sim.forward_simulate_traced(wl.robot, wl.starts, wl.targets, True, config_capacity=CONFIG_CAPACITY)
        else:
            res, buf = sim.forward_simulate_traced_mutable(wl.robot, wl.starts, wl.targets, True, sc.controller_state.copy(),
                                                           config_capacity=CONFIG_CAPACITY)
        errors = res["error_flags"]
    finally:
        sim.close()
    assert not np.any(errors), np.unique(errors)
    return buf


def _diff(ref, record, wrapped, B):
    """|reference - record| per element as floats, the wrapped elements modulo 2 pi"""
    d = ref - B.array(record)
    for k in wrapped:
        d[k] = H.wrap(d[k], B)
    return np.abs(H.to_float(d))


def replay_scene(sc, buf, B=H.DEFAULT):
    """Replays the traced run `buf` of the scene (module docstring); returns its figures."""
    t0 = time.time()
    wl, robot = sc.wl, sc.wl.robot
    n, D = len(wl.starts), robot.num_dofs
    assert np.all(buf.num_configs <= buf.config_capacity) and np.all(buf.num_steps <= buf.step_capacity), "trace truncated"
    ref = A.ActuationReference(robot, 1.0 / wl.controller_frequency, B)
    key = A.call_key(int(wl.seed), int(sc.call_index))
    slots = NOISE_SLOTS // D
    stats = {"steps": 0, "steps_skipped": 0, "microsteps": 0, "skipped": 0, "worst_input": 0.0, "worst_step": 0.0, "worst_post": 0.0,
             "refilled": 0, "ragged": 0, "arms": [0, 0], "max_abs": 0.0, "wrapped": 0, "limited": 0,
             "unsaturated": 0, "state_shows": 0}
    failures = []
    for i in range(n):
        start = H.to_float(H.apply_control_input(robot, wl.starts[i], np.zeros(D), B))  # ResetPosition's SetPosition
        target = wl.targets[i] if len(wl.targets) == n else wl.targets[0]
        tags = buf.config_tags[i, :int(buf.num_configs[i])]
        state = ref.zero_state() if sc.controller_state is None else ref.state_from(sc.controller_state[i])
        zeroed = ref.zero_state()  # a mutable-robot call: what a controller that ignored the passed-in state would do
        for s in range(int(buf.num_steps[i])):
            where = f"particle {i} step {s}"
            records = np.nonzero(tags[:, 0] == s)[0]
            assert len(records), f"{sc.name}: {where} has no record"
            q0 = buf.configs[i, records[0] - 1] if records[0] > 0 else start
            # (a)
            candidates = [ref.controller_step(state, q0, target)]
            if i in sc.either_sign:
                candidates.append(ref.controller_step(state, q0, target, flip=True))
            recorded = buf.step_inputs[i, s, 0]
            ratios = [float(np.max(_diff(ci, recorded, [], B) / np.maximum(bound, 1e-300))) for ci, bound, _, _ in candidates]
            best = int(np.argmin(ratios))
            ci, bound, near, state = candidates[best]
            stats["steps"] += 1
            stats["unsaturated"] += state["unsaturated"]
            if sc.controller_state is not None:
                ci0, bound0, _, zeroed = ref.controller_step(zeroed, q0, target)
                stats["state_shows"] += int(np.any(_diff(ci, H.to_float(ci0), [], B) > bound + bound0))
            if near:
                stats["steps_skipped"] += 1
            else:
                stats["worst_input"] = max(stats["worst_input"], ratios[best])
                if ratios[best] > 1.0:
                    failures.append(f"{where}: control_input off by {ratios[best]:.3g} of its bound "
                                    f"({_diff(ci, recorded, [], B).max():.3e})")
            # (b)
            count = int(buf.step_microsteps[i, s])
            step_input = buf.step_inputs[i, s, 1]
            quotient = B.array(recorded) / count
            r = float(np.max(_diff(quotient, step_input, [], B) / np.maximum(U * np.abs(step_input), 1e-300)))
            stats["worst_step"] = max(stats["worst_step"], r)
            if r > 1.0:
                failures.append(f"{where}: control_input_step is not control_input / {count}")
            posts = [k for k in records if tags[k, 2] == TRACE_POST_ACTION]
            ended = int(tags[records[-1], 2]) in (TRACE_RESOLVE_FAILED, TRACE_CONTACT_STOP)
            if [int(tags[k, 1]) for k in posts] != list(range(len(posts))) or (len(posts) != count and not ended) or len(posts) > count:
                failures.append(f"{where}: {len(posts)} post-action records for {count} microsteps")
            stats["refilled"] += int(slots > 0 and len(posts) > slots)
            stats["ragged"] += int(slots > 1 and count % slots != 0)
            # (c)
            for m, k in enumerate(posts):
                previous = buf.configs[i, k - 1] if k > 0 else start
                nxt, tol, near_draw, arms, wrapped = ref.noisy_apply(previous, step_input, key, sc.first_particle_id + i, s, m)
                stats["microsteps"] += 1
                for a in arms:
                    if a is not None:
                        stats["arms"][a] += 1
                if near_draw:
                    stats["skipped"] += 1
                    continue
                d = _diff(nxt, buf.configs[i, k], wrapped, B)
                r = float(np.max(d / tol))
                stats["worst_post"] = max(stats["worst_post"], r)
                stats["max_abs"] = max(stats["max_abs"], float(d.max()))
                for e, (kind, lo, hi) in enumerate(ref.kinds):
                    stats["wrapped"] += int(kind == "wrap" and abs(previous[e] + step_input[e]) > np.pi)
                    stats["limited"] += int(kind == "limit" and buf.configs[i, k, e] in (lo, hi))
                if r > 1.0:
                    failures.append(f"{where} microstep {m}: post-action configuration off by {r:.3g} of its bound ({d.max():.3e})")
    stats["seconds"] = time.time() - t0
    print(f"{sc.name}: {stats['steps']} controller steps ({stats['steps_skipped']} near), {stats['microsteps']} microsteps "
          f"({stats['skipped']} near); worst ratio to the bound: control_input {stats['worst_input']:.3f}, control_input_step "
          f"{stats['worst_step']:.3f}, post-action {stats['worst_post']:.3f} (largest difference {stats['max_abs']:.2e}); "
          f"{stats['refilled']} steps refill the noise buffer, {stats['ragged']} end inside one; noise bound decided by "
          f"prop |real| {stats['arms'][0]} times, by min vmax {stats['arms'][1]}; {stats['wrapped']} wraps, {stats['limited']} limit "
          f"clamps; {stats['unsaturated']} dof-steps inside the velocity clamp"
          + (f", the passed-in PID state shows in {stats['state_shows']} steps" if sc.controller_state is not None else "")
          + f"; {stats['seconds']:.1f} s")
    assert not failures, f"{sc.name}: " + "; ".join(failures[:6]) + (f" (+{len(failures) - 6} more)" if len(failures) > 6 else "")
    assert stats["steps"] > 0 and stats["microsteps"] > 0
    assert stats["steps_skipped"] == 0, f"{sc.name}: {stats['steps_skipped']} controller steps near a clamp"
    assert stats["skipped"] <= SKIP_CAP * stats["microsteps"], f"{sc.name}: {stats['skipped']} of {stats['microsteps']} microsteps near"
    if robot.robot_type == _capi.ROBOT_LINKED if sc.refill is None else sc.refill:
        assert stats["refilled"] > 0, f"{sc.name}: no step of more than floor(64 / {D}) = {slots} microsteps"
        if slots > 1:  # every count is a multiple of 1
            assert stats["ragged"] > 0, f"{sc.name}: every step's count is a multiple of {slots}"
    assert stats["limited"] > 0 or not sc.limits, f"{sc.name}: no post-action value on a joint limit"
    assert stats["wrapped"] > 0 or not sc.wraps, f"{sc.name}: no post-action value wrapped"
    assert stats["unsaturated"] > 0 or not sc.controller, f"{sc.name}: every PID term of every step is clamped to the velocity limit"
    if sc.controller_state is not None:
        assert stats["state_shows"] > 0, f"{sc.name}: the passed-in PID state changes no control_input by more than its bound"
    if sc.both_arms:
        assert min(stats["arms"]) > 0, f"{sc.name}: the noise bound's max was decided {stats['arms']} times by its two arms"
    return stats
