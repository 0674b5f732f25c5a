"""TEST INFRASTRUCTURE ONLY — Python binding of the CPU oracle (oracle/_build/liboracle.so).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this package; it is the checker and the reported CPU baseline, never the thing
measured or shipped.  The product (fast_kinematic_simulator_amd) never imports it.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import subprocess
from ctypes import POINTER, c_double, c_int32, c_uint8, c_uint32, c_uint64, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "liboracle.so")
RNG_COUNTER, RNG_REFERENCE = 0, 1
_LIB = None


def build(force: bool = False) -> str:
    """Compile the oracle with its Makefile (g++, OpenMP)."""
    cmd = ["make", "-C", HERE] + (["-B"] if force else [])
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        build()  # make: a no-op when liboracle.so is newer than its sources
        _LIB = _load(LIB_PATH)
    return _LIB


AUDIT_VARIANTS = ("v4seq", "seqsum", "libm", "fma")


@contextlib.contextmanager
def audit_variant(name):
    """Run the oracle entry points on a restatement-audit build (oracle/Makefile `audit`,
    DESIGN.md §2.3) inside the block.  Never a parity oracle."""
    global _LIB
    assert name in AUDIT_VARIANTS, name
    path = os.path.join(HERE, "_build", "liboracle_%s.so" % name)
    subprocess.run(["make", "-C", HERE, "audit"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    saved = lib()
    _LIB = _load(path)
    try:
        yield _LIB
    finally:
        _LIB = saved


def _load(path):
    from fast_kinematic_simulator_amd import _capi as C  # struct layouts only (the ABI types)

    L = ctypes.CDLL(path)
    L.oracle_forward_simulate.restype = c_int32
    L.oracle_forward_simulate.argtypes = [
        POINTER(C.Environment), POINTER(C.SolverParams), c_double, c_uint64, c_uint64, POINTER(C.RobotDesc),
        POINTER(c_double), c_uint64, POINTER(c_double), c_uint64, c_uint64, c_int32, c_int32, c_int32, POINTER(c_double),
        POINTER(c_uint8), POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32), POINTER(C.Statistics),
        POINTER(C.CallCounters), c_int32, POINTER(c_double)]
    L.oracle_check_config_collision.restype = c_int32
    L.oracle_check_config_collision.argtypes = [
        POINTER(C.Environment), POINTER(C.SolverParams), POINTER(C.RobotDesc), POINTER(c_double), c_uint64, c_double,
        c_int32, POINTER(c_uint8), POINTER(c_uint32), POINTER(c_uint64)]
    L.oracle_forward_simulate_traced.restype = c_int32
    L.oracle_forward_simulate_traced.argtypes = [
        POINTER(C.Environment), POINTER(C.SolverParams), c_double, c_uint64, c_uint64, POINTER(C.RobotDesc),
        POINTER(c_double), c_uint64, POINTER(c_double), c_uint64, c_int32, c_int32, POINTER(c_double), POINTER(c_uint8),
        POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32), POINTER(C.Trace), c_uint64]
    L.oracle_forward_simulate_traced_individual.restype = c_int32
    L.oracle_forward_simulate_traced_individual.argtypes = L.oracle_forward_simulate_traced.argtypes + [c_int32]
    L.oracle_philox4x32_10.restype = None
    L.oracle_philox4x32_10.argtypes = [POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]
    L.oracle_pid_sequence.restype = None
    L.oracle_pid_sequence.argtypes = [c_double, c_double, c_double, c_double, POINTER(c_double), POINTER(c_double), c_int32,
                                      POINTER(c_double)]
    L.oracle_counter_truncated_normal.restype = c_double
    L.oracle_counter_truncated_normal.argtypes = [c_uint64, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, POINTER(c_uint32)]
    L.oracle_qr_info.restype = None
    L.oracle_qr_info.argtypes = [POINTER(c_double), c_uint64, c_uint64, POINTER(c_double), POINTER(c_double), POINTER(c_uint64),
                                 POINTER(c_uint64)]
    L.oracle_capture_systems.restype = None
    L.oracle_capture_systems.argtypes = [c_uint64, c_uint64, c_uint64]
    L.oracle_captured_systems.restype = c_uint64
    L.oracle_captured_systems.argtypes = [POINTER(c_uint64), POINTER(c_uint64)]
    L.oracle_copy_captured.restype = None
    L.oracle_copy_captured.argtypes = [POINTER(c_double), POINTER(c_double), POINTER(c_uint64)]
    L.oracle_qr_solve.restype = None
    L.oracle_qr_solve.argtypes = [POINTER(c_double), c_uint64, c_uint64, POINTER(c_double), POINTER(c_double)]
    L.oracle_estimate_distance.restype = None
    L.oracle_estimate_distance.argtypes = [POINTER(C.Environment), POINTER(c_double), c_uint64, POINTER(c_double),
                                           POINTER(c_uint8), POINTER(ctypes.c_float)]
    L.oracle_link_transforms.restype = c_int32
    L.oracle_link_transforms.argtypes = [POINTER(C.RobotDesc), POINTER(c_double), POINTER(c_double)]
    L.oracle_apply_control_input.restype = c_int32
    L.oracle_apply_control_input.argtypes = [POINTER(C.RobotDesc), POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    L.oracle_robot_steps.restype = c_int32
    L.oracle_robot_steps.argtypes = [POINTER(C.RobotDesc), POINTER(c_double), POINTER(c_double), c_double, c_uint32, c_uint64,
                                     c_uint64, POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    L.oracle_point_jacobian.restype = c_int32
    L.oracle_point_jacobian.argtypes = [POINTER(C.RobotDesc), POINTER(c_double), c_int32, POINTER(c_double), POINTER(c_double)]
    L.oracle_se3_exp.restype = None
    L.oracle_se3_exp.argtypes = [POINTER(c_double), POINTER(c_double)]
    L.oracle_se3_log.restype = None
    L.oracle_se3_log.argtypes = [POINTER(c_double), POINTER(c_double)]
    L.oracle_max_threads.restype = c_int32
    L.oracle_portable_math.restype = None
    L.oracle_portable_math.argtypes = [c_int32, POINTER(c_double), POINTER(c_double), c_uint64, POINTER(c_double)]
    return L


def _p(a, t):
    return a.ctypes.data_as(POINTER(t))


def forward_simulate(env, robot, solver, frequency, seed, starts, targets, allow_contacts=True, call_index=0,
                     first_particle_id=0, rng_mode=RNG_COUNTER, threads=0, individual_jacobians=False,
                     controller_state=None):
    """ForwardSimulateRobots on the CPU oracle.  Returns a dict like the HIP path.
    individual_jacobians: the simulate_with_individual_jacobians constructor flag (SPCS:420).
    controller_state: None (ResetPosition zeroes the PIDs) or an (n, 2D) float64 array of PID
    states, updated in place (ForwardSimulateMutableRobot, SPCS:843-919)."""
    L = lib()
    from fast_kinematic_simulator_amd import _capi as C

    W = robot.config_width
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(-1, W))
    targets = np.ascontiguousarray(np.asarray(targets, dtype=np.float64).reshape(-1, W))
    n = starts.shape[0]
    env_c, keep_env = env.to_c()
    desc, keep_robot = robot.to_c()
    params = solver.to_c()
    out = np.zeros((n, W))
    coll = np.zeros(n, dtype=np.uint8)
    micro = np.zeros(n, dtype=np.uint32)
    res = np.zeros(n, dtype=np.uint32)
    err = np.zeros(n, dtype=np.uint32)
    stats = C.Statistics()
    cc = C.CallCounters()
    st = L.oracle_forward_simulate(ctypes.byref(env_c), ctypes.byref(params), float(frequency), c_uint64(int(seed)),
                                   c_uint64(int(call_index)), ctypes.byref(desc), _p(starts, c_double), n,
                                   _p(targets, c_double), targets.shape[0], int(first_particle_id), 1 if allow_contacts else 0,
                                   int(rng_mode), int(threads), _p(out, c_double), _p(coll, c_uint8), _p(micro, c_uint32),
                                   _p(res, c_uint32), _p(err, c_uint32), ctypes.byref(stats), ctypes.byref(cc),
                                   1 if individual_jacobians else 0,
                                   _p(controller_state, c_double) if controller_state is not None else None)
    del keep_env, keep_robot
    if st != 0:
        raise RuntimeError(f"oracle_forward_simulate failed ({st})")
    return {"positions": out, "collided": coll.astype(bool), "microsteps": micro, "resolver_iterations": res, "error_flags": err,
            "statistics": stats.as_dict(), "counters": cc.as_dict()}


def forward_simulate_traced(env, robot, solver, frequency, seed, starts, targets, allow_contacts=True, call_index=0,
                            step_capacity=None, config_capacity=4096, threads=0, first_particle_id=0,
                            individual_jacobians=False):
    """ForwardSimulateRobot with enable_tracing (SPCS:824-829) per particle, counter RNG.
    individual_jacobians: the simulate_with_individual_jacobians constructor flag (SPCS:420).
    Returns (result dict, fast_kinematic_simulator_amd.trace.TraceBuffers)."""
    L = lib()
    from fast_kinematic_simulator_amd.trace import TraceBuffers

    W, D = robot.config_width, robot.num_dofs
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(-1, W))
    targets = np.ascontiguousarray(np.asarray(targets, dtype=np.float64).reshape(-1, W))
    n = starts.shape[0]
    if step_capacity is None:
        step_capacity = max(1, int(solver.forward_simulation_time * frequency))
    buf = TraceBuffers(n, D, W, step_capacity, config_capacity)
    tr = buf.to_c()
    env_c, keep_env = env.to_c()
    desc, keep_robot = robot.to_c()
    params = solver.to_c()
    out = np.zeros((n, W))
    coll = np.zeros(n, dtype=np.uint8)
    micro = np.zeros(n, dtype=np.uint32)
    res = np.zeros(n, dtype=np.uint32)
    err = np.zeros(n, dtype=np.uint32)
    args = [ctypes.byref(env_c), ctypes.byref(params), float(frequency), c_uint64(int(seed)), c_uint64(int(call_index)),
            ctypes.byref(desc), _p(starts, c_double), n, _p(targets, c_double), targets.shape[0], 1 if allow_contacts else 0,
            int(threads), _p(out, c_double), _p(coll, c_uint8), _p(micro, c_uint32), _p(res, c_uint32), _p(err, c_uint32),
            ctypes.byref(tr), c_uint64(int(first_particle_id))]
    # the stacked solve stays on the entry it always used (the sanitizer driver calls it too)
    st = L.oracle_forward_simulate_traced_individual(*args, 1) if individual_jacobians else L.oracle_forward_simulate_traced(*args)
    del keep_env, keep_robot
    if st != 0:
        raise RuntimeError(f"oracle_forward_simulate_traced failed ({st})")
    return ({"positions": out, "collided": coll.astype(bool), "microsteps": micro, "resolver_iterations": res,
             "error_flags": err}, buf)


def check_config_collision(env, robot, solver, configs, inflation_ratio=0.0, threads=0):
    """CheckConfigCollision (SPCS:1398-1416) for each configuration on the CPU oracle."""
    L = lib()
    W = robot.config_width
    configs = np.ascontiguousarray(np.asarray(configs, dtype=np.float64).reshape(-1, W))
    n = configs.shape[0]
    env_c, keep_env = env.to_c()
    desc, keep_robot = robot.to_c()
    params = solver.to_c()
    coll = np.zeros(n, dtype=np.uint8)
    err = np.zeros(n, dtype=np.uint32)
    nbytes = np.zeros(n, dtype=np.uint64)
    st = L.oracle_check_config_collision(ctypes.byref(env_c), ctypes.byref(params), ctypes.byref(desc), _p(configs, c_double), n,
                                         float(inflation_ratio), int(threads), _p(coll, c_uint8), _p(err, c_uint32),
                                         _p(nbytes, c_uint64))
    del keep_env, keep_robot
    if st != 0:
        raise RuntimeError(f"oracle_check_config_collision failed ({st})")
    return {"collided": coll.astype(bool), "error_flags": err, "sdf_bytes": nbytes}


def philox(ctr, key):
    L = lib()
    c = np.array(ctr, dtype=np.uint32)
    k = np.array(key, dtype=np.uint32)
    o = np.zeros(4, dtype=np.uint32)
    L.oracle_philox4x32_10(_p(c, c_uint32), _p(k, c_uint32), _p(o, c_uint32))
    return [int(v) for v in o]


def pid_sequence(kp, ki, kd, iclamp, errors, dts):
    L = lib()
    e = np.ascontiguousarray(errors, dtype=np.float64)
    d = np.ascontiguousarray(dts, dtype=np.float64)
    o = np.zeros(len(e))
    L.oracle_pid_sequence(kp, ki, kd, iclamp, _p(e, c_double), _p(d, c_double), len(e), _p(o, c_double))
    return o


def truncated_normal(seed, call_index, particle, step, micro, dof):
    err = c_uint32(0)
    v = lib().oracle_counter_truncated_normal(seed, call_index, particle, step, micro, dof, ctypes.byref(err))
    return v, err.value


def qr_solve(J, b):
    J = np.ascontiguousarray(J, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(J.shape[1])
    lib().oracle_qr_solve(_p(J, c_double), J.shape[0], J.shape[1], _p(b, c_double), _p(x, c_double))
    return x


def qr_info(J, b):
    """The oracle's ColPivHouseholderQR of J (SPCS:1994): (basic solution x, permutation
    perm with perm[i] = the original column of pivot i, number of nonzero pivots)."""
    J = np.ascontiguousarray(J, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    D = J.shape[1]
    x = np.zeros(D)
    perm = np.zeros(D, dtype=np.uint64)
    nz = c_uint64(0)
    lib().oracle_qr_info(_p(J, c_double), J.shape[0], D, _p(b, c_double), _p(x, c_double), _p(perm, c_uint64), ctypes.byref(nz))
    return x, perm.astype(np.int64), int(nz.value)


@contextlib.contextmanager
def captured_systems(max_systems, stride=1, max_rows=64):
    """Record the stacked least-squares systems (J, b) the simulator solves inside the block
    (every `stride`-th with at most `max_rows` rows); yields a list filled on exit."""
    L = lib()
    out = []
    L.oracle_capture_systems(int(max_systems), int(stride), int(max_rows))
    try:
        yield out
    finally:
        nj, nb = c_uint64(0), c_uint64(0)
        n = int(L.oracle_captured_systems(ctypes.byref(nj), ctypes.byref(nb)))
        J = np.zeros(nj.value)
        b = np.zeros(nb.value)
        shape = np.zeros(2 * n, dtype=np.uint64)
        if n:
            L.oracle_copy_captured(_p(J, c_double), _p(b, c_double), _p(shape, c_uint64))
        L.oracle_capture_systems(0, 1, 0)
        oj = ob = 0
        for k in range(n):
            r, c = int(shape[2 * k]), int(shape[2 * k + 1])
            out.append((J[oj:oj + r * c].reshape(r, c).copy(), b[ob:ob + r].copy()))
            oj += r * c
            ob += r


def estimate_distance(env, points):
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 4))
    env_c, keep = env.to_c()
    d = np.zeros(len(pts))
    inb = np.zeros(len(pts), dtype=np.uint8)
    near = np.zeros(len(pts), dtype=np.float32)
    lib().oracle_estimate_distance(ctypes.byref(env_c), _p(pts, c_double), len(pts), _p(d, c_double), _p(inb, c_uint8),
                                   _p(near, ctypes.c_float))
    return d, inb.astype(bool), near


def link_transforms(robot, config):
    desc, keep = robot.to_c()
    cfg = np.ascontiguousarray(config, dtype=np.float64)
    out = np.zeros((len(robot.geometry_points), 12))
    lib().oracle_link_transforms(ctypes.byref(desc), _p(cfg, c_double), _p(out, c_double))
    return out


def apply_control_input(robot, config, control_input):
    """SetPosition + clean ApplyControlInput (TNUVA:538-566) on the CPU."""
    desc, keep = robot.to_c()
    cfg = np.ascontiguousarray(config, dtype=np.float64)
    u = np.ascontiguousarray(control_input, dtype=np.float64)
    out = np.zeros(robot.config_width)
    lib().oracle_apply_control_input(ctypes.byref(desc), _p(cfg, c_double), _p(u, c_double), _p(out, c_double))
    return out


def robot_steps(robot, start, target, controller_interval, steps, seed, noisy_mask=0):
    """One robot stepped by hand: GenerateControlAction + ApplyControlInput per step (noisy on
    the steps set in noisy_mask, std::mt19937_64(seed)).  Returns (controls, configs, pid)."""
    desc, keep = robot.to_c()
    W, D = robot.config_width, robot.num_dofs
    s = np.ascontiguousarray(start, dtype=np.float64)
    t = np.ascontiguousarray(target, dtype=np.float64)
    u = np.zeros((steps, D))
    q = np.zeros((steps, W))
    pid = np.zeros(2 * D)
    st = lib().oracle_robot_steps(ctypes.byref(desc), _p(s, c_double), _p(t, c_double), float(controller_interval), int(steps),
                                  c_uint64(int(seed)), c_uint64(int(noisy_mask)), _p(u, c_double), _p(q, c_double),
                                  _p(pid, c_double))
    del keep
    if st != 0:
        raise RuntimeError(f"oracle_robot_steps failed ({st})")
    return u, q, pid


def point_jacobian(robot, config, geometry, point):
    desc, keep = robot.to_c()
    cfg = np.ascontiguousarray(config, dtype=np.float64)
    p = np.ascontiguousarray(point, dtype=np.float64)
    out = np.zeros(3 * robot.num_dofs)
    lib().oracle_point_jacobian(ctypes.byref(desc), _p(cfg, c_double), int(geometry), _p(p, c_double), _p(out, c_double))
    return out.reshape(3, robot.num_dofs)


def se3_exp(twist):
    t = np.ascontiguousarray(twist, dtype=np.float64)
    o = np.zeros(12)
    lib().oracle_se3_exp(_p(t, c_double), _p(o, c_double))
    return o


def se3_log(pose):
    p = np.ascontiguousarray(pose, dtype=np.float64)
    o = np.zeros(6)
    lib().oracle_se3_log(_p(p, c_double), _p(o, c_double))
    return o


def portable_math(fn, x, y=None):
    """fn: 0 sin, 1 cos, 2 log, 3 atan, 4 atan2(x, y), 5 wrap, 6 fmod_two_pi, 7 wrap_revolute
    (include/fks_portable_math.h)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y if y is not None else np.zeros_like(x), dtype=np.float64)
    o = np.zeros_like(x)
    lib().oracle_portable_math(int(fn), _p(x, c_double), _p(y, c_double), len(x), _p(o, c_double))
    return o
