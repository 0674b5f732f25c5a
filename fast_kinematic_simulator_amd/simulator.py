"""Host-side mirror of the reference simulator interface over the C-ABI.

Mirrors ``simple_particle_contact_simulator::SimpleParticleContactSimulator``
(SPCS:371-1999) as seen through ``uncertainty_planning_core``'s
``SimulatorInterface`` and the ``fast_kinematic_simulator`` factories
(FKS.hpp:11-22, FKS.cpp:4-71).  Batch calls run on the GPU through
``libfks_hip.so``; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, fields
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _capi
from .environment import DeviceEnvironment, SimulatorEnvironment
from .robots import RobotDescription
from .trace import ForwardSimulationStepTrace, TraceBuffers

# the outputs of a summary call, in the order of fks_cluster_summary
SUMMARY_OUTPUTS = ("order", "members", "count", "begin", "expectation", "variances", "variance", "reached")


@dataclass
class SimulatorSolverParameters:
    """SimulatorSolverParameters with the defaults of SPCS:357-368."""

    forward_simulation_time: float = 1.0
    simulation_shortcut_distance: float = 0.0
    environment_collision_check_tolerance: float = 0.001
    resolve_correction_step_scaling_decay_rate: float = 0.5
    resolve_correction_initial_step_size: float = 1.0
    resolve_correction_min_step_scaling: float = 0.03125
    max_resolver_iterations: int = 25
    resolve_correction_step_scaling_decay_iterations: int = 5
    failed_resolves_end_motion: bool = True

    def to_c(self) -> _capi.SolverParams:
        p = _capi.SolverParams()
        for f in fields(self):
            v = getattr(self, f.name)
            setattr(p, f.name, int(v) if isinstance(v, (bool, int)) and not isinstance(v, float) else v)
        return p


def get_default_solver_parameters() -> SimulatorSolverParameters:
    """fast_kinematic_simulator::GetDefaultSolverParameters (FKS.hpp:13-16)."""
    return SimulatorSolverParameters()


@dataclass
class SimulationResult:
    """simple_simulator_interface::SimulationResult(reached, target, collided, true) (SPCS:918)."""

    result_config: np.ndarray
    target_config: np.ndarray
    did_contact: bool
    outcome_is_valid: bool = True
    microsteps: int = 0
    resolver_iterations: int = 0
    error_flags: int = 0


class HipParticleContactSimulator:
    """SimpleParticleContactSimulator on one MI355X.  The stacked-Jacobian resolver
    is always used, as the factories hard-wire (FKS.cpp:22,45,68)."""

    def __init__(self, environment: SimulatorEnvironment, solver_config: SimulatorSolverParameters,
                 simulation_controller_frequency: float, prng_seed: int, debug_level: int = 0, device: int = 0):
        self._lib = _capi.lib()
        self.environment = environment
        self.solver_config = solver_config
        self.simulation_controller_frequency = float(simulation_controller_frequency)
        self.prng_seed = int(prng_seed)
        params = solver_config.to_c()
        ctx = ctypes.c_void_p()
        if isinstance(environment, DeviceEnvironment):
            # device-resident GPU build: SDF + normal CSR copied device to device (fks_create_from_device_env)
            self._env_keep = None
            st = self._lib.fks_create_from_device_env(environment.handle, ctypes.byref(params),
                                                      self.simulation_controller_frequency,
                                                      ctypes.c_uint64(self.prng_seed & 0xFFFFFFFFFFFFFFFF), int(debug_level),
                                                      ctypes.byref(ctx))
            _capi.check(st, None, "fks_create_from_device_env")
        else:
            env_c, self._env_keep = environment.to_c()
            st = self._lib.fks_create(ctypes.byref(env_c), ctypes.byref(params), self.simulation_controller_frequency,
                                      ctypes.c_uint64(self.prng_seed & 0xFFFFFFFFFFFFFFFF), int(debug_level), int(device),
                                      ctypes.byref(ctx))
            _capi.check(st, None, "fks_create")
        self._ctx = ctx
        self._robot_key = None
        self._robot = None

    # ---- lifetime ----
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.fks_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference interface ----
    def get_debug_level(self) -> int:
        return int(self._lib.fks_get_debug_level(self._ctx))

    def set_debug_level(self, debug_level: int) -> int:
        return int(self._lib.fks_set_debug_level(self._ctx, int(debug_level)))

    def get_statistics(self) -> dict:
        s = _capi.Statistics()
        _capi.check(self._lib.fks_get_statistics(self._ctx, ctypes.byref(s)), self._ctx, "fks_get_statistics")
        return s.as_dict()

    def reset_statistics(self):
        _capi.check(self._lib.fks_reset_statistics(self._ctx), self._ctx, "fks_reset_statistics")

    def reset_generators(self, prng_seed: int):
        _capi.check(self._lib.fks_reset_generators(self._ctx, ctypes.c_uint64(int(prng_seed))), self._ctx, "reset")

    def set_call_index(self, call_index: int):
        _capi.check(self._lib.fks_set_call_index(self._ctx, ctypes.c_uint64(int(call_index))), self._ctx, "call index")

    def get_call_index(self) -> int:
        return int(self._lib.fks_get_call_index(self._ctx))

    def last_call_counters(self) -> dict:
        c = _capi.CallCounters()
        _capi.check(self._lib.fks_get_last_call_counters(self._ctx, ctypes.byref(c)), self._ctx, "counters")
        return c.as_dict()

    def total_counters(self) -> dict:
        c = _capi.CallCounters()
        _capi.check(self._lib.fks_get_total_counters(self._ctx, ctypes.byref(c)), self._ctx, "counters")
        return c.as_dict()

    def reset_total_counters(self):
        _capi.check(self._lib.fks_reset_total_counters(self._ctx), self._ctx, "counters")

    def phase_cycles(self, total: bool = True) -> dict:
        """Shader-clock cycles per kernel phase (fks_get_phase_cycles), summed over waves."""
        arr = (ctypes.c_uint64 * _capi.NUM_PHASES)()
        _capi.check(self._lib.fks_get_phase_cycles(self._ctx, 1 if total else 0, arr), self._ctx, "phase cycles")
        return {name: int(arr[i]) for i, name in enumerate(_capi.PHASE_NAMES)}

    def set_segment_steps(self, controller_steps: int = 0):
        """Controller steps per scheduling segment of a batch (fks_set_segment_steps;
        0 = automatic).  Results do not depend on it."""
        _capi.check(self._lib.fks_set_segment_steps(self._ctx, int(controller_steps)), self._ctx, "segment steps")

    def set_segment_policy(self, heavy_resolver_per_step: int = 2, heavy_priority: int = 2):
        """Scheduling policy of segmented batches (fks_set_segment_policy): contact-heavy
        segments keep their wave and raise its issue priority.  Results do not depend on it."""
        _capi.check(self._lib.fks_set_segment_policy(self._ctx, int(heavy_resolver_per_step), int(heavy_priority)), self._ctx,
                    "segment policy")

    def set_segment_heavy_relative(self, times_mean: int = 3):
        """A heavy segment must also exceed times_mean x the batch's running mean resolver
        iterations per segment (fks_set_segment_heavy_relative; 0 = off).  Results do not depend on it."""
        _capi.check(self._lib.fks_set_segment_heavy_relative(self._ctx, int(times_mean)), self._ctx, "segment heavy relative")

    def set_small_batch_kernel(self, enabled: bool = True):
        """Batches that fit the low-occupancy instantiation's resident waves run it
        (fks_set_small_batch_kernel; default on).  Results do not depend on it."""
        _capi.check(self._lib.fks_set_small_batch_kernel(self._ctx, 1 if enabled else 0), self._ctx, "small batch kernel")

    def set_cooperative_waves(self, enabled: bool = True):
        """Batches of at most launch_info()["cooperative_resident_particles"] particles run one
        particle per workgroup, its environment checks and correction passes shared over the
        workgroup's waves (fks_set_cooperative_waves; default off: slower on the measured
        workloads).  Results do not depend on it."""
        _capi.check(self._lib.fks_set_cooperative_waves(self._ctx, 1 if enabled else 0), self._ctx, "cooperative waves")

    def set_specialization(self, enabled=True):
        """Run the plain throughput simulation of this robot (and of every robot set later) on a
        kernel compiled at run time for its shape (fks_set_specialization: hiprtc, cached per
        process and on disk).  On by default, built at the first call that runs it; enabling
        it builds the current robot's kernel now.  Results do not depend on it; raises FksError
        with the compiler log when the current robot's kernel cannot be built (the calls then
        keep the generic kernel, and specialization()["failed"] says so).  enabled may also be
        an fks_specialization_mode: _capi.SPECIALIZE_NO_PROOFS builds the validation kernel with
        every skip proof compiled out (same results, slower)."""
        mode = int(enabled) if not isinstance(enabled, bool) else (_capi.SPECIALIZE_ON if enabled else _capi.SPECIALIZE_OFF)
        _capi.check(self._lib.fks_set_specialization(self._ctx, mode), self._ctx, "specialization")

    def launch_info(self) -> dict:
        """fks_get_launch_info: the layout fks_set_robot chose and the kernel of the last call."""
        info = _capi.LaunchInfo()
        _capi.check(self._lib.fks_get_launch_info(self._ctx, ctypes.byref(info)), self._ctx, "launch info")
        return info.as_dict()

    def specialization(self) -> dict:
        """fks_get_specialization: enabled (mode), active, pending, from_cache, compile_seconds, launches,
        shape, failed, message"""
        info = _capi.SpecializationInfo()
        _capi.check(self._lib.fks_get_specialization(self._ctx, ctypes.byref(info)), self._ctx, "specialization")
        return info.as_dict()

    def prepare_batched_specialization(self):
        """Build (or fetch from the caches) the current robot's batched module now: the shaped
        kernels of path, job and path-job batches (fks_prepare_batched_specialization), and
        switch those batches to it.  After set_batched_specialization(True) alone it is built at
        the first such batch that outgrows the small-batch grid or runs in segments.  Raises
        FksError with the compiler log when it cannot be built; the batches then keep the generic
        kernels, with the same results."""
        _capi.check(self._lib.fks_prepare_batched_specialization(self._ctx), self._ctx, "batched specialization")

    def set_batched_specialization(self, enabled: bool = True):
        """True runs path, job and path-job batches on the robot's batched shaped module
        (fks_set_batched_specialization; off by default: the batches then run the generic
        kernels while plain calls stay on the shaped one).  Results do not depend on it."""
        _capi.check(self._lib.fks_set_batched_specialization(self._ctx, 1 if enabled else 0), self._ctx, "batched specialization")

    def batched_specialization(self) -> dict:
        """fks_get_batched_specialization: specialization()'s fields for the batched module (its
        shape ends in "-b"; enabled is set_batched_specialization's value)."""
        info = _capi.SpecializationInfo()
        _capi.check(self._lib.fks_get_batched_specialization(self._ctx, ctypes.byref(info)), self._ctx, "batched specialization")
        return info.as_dict()

    def set_individual_jacobians(self, simulate_with_individual_jacobians: bool):
        """The simulate_with_individual_jacobians constructor flag of the reference class
        (SPCS:420-423, 1629): True selects ComputeResolverCorrectionStepIndividualJacobians
        (SPCS:1966-1988) instead of the stacked solve the factories hard-wire (FKS.cpp:22)."""
        _capi.check(self._lib.fks_set_individual_jacobians(self._ctx, 1 if simulate_with_individual_jacobians else 0), self._ctx,
                    "individual jacobians")

    def launch_geometry(self) -> dict:
        """Resident waves of the persistent simulation grid and LDS bytes per workgroup
        (fks_get_launch_geometry) for the robot set last."""
        waves, lds = ctypes.c_uint32(0), ctypes.c_uint64(0)
        _capi.check(self._lib.fks_get_launch_geometry(self._ctx, ctypes.byref(waves), ctypes.byref(lds)), self._ctx,
                    "launch geometry")
        return {"resident_waves": int(waves.value), "lds_bytes_per_group": int(lds.value)}

    def set_robot(self, robot: RobotDescription):
        key = id(robot)
        if self._robot_key == key and self._robot is robot:
            return
        desc, keep = robot.to_c()
        _capi.check(self._lib.fks_set_robot(self._ctx, ctypes.byref(desc)), self._ctx, "fks_set_robot")
        del keep
        self._robot_key = key
        self._robot = robot

    def forward_simulate_arrays(self, robot: RobotDescription, start_positions, target_positions, allow_contacts: bool,
                                reverse: bool = False) -> dict:
        """Batch call with numpy arrays: starts (n, W), targets (1 or n, W)."""
        self.set_robot(robot)
        W = robot.config_width
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        targets = np.ascontiguousarray(np.asarray(target_positions, dtype=np.float64).reshape(-1, W))
        n = starts.shape[0]
        if n > 0 and targets.shape[0] not in (1, n):
            raise ValueError("target_positions must hold 1 or len(start_positions) configurations (SPCS:792)")
        out = np.zeros((n, W), dtype=np.float64)
        collided = np.zeros(n, dtype=np.uint8)
        micro = np.zeros(n, dtype=np.uint32)
        resolver = np.zeros(n, dtype=np.uint32)
        errors = np.zeros(n, dtype=np.uint32)
        fn = self._lib.fks_reverse_simulate if reverse else self._lib.fks_forward_simulate
        st = fn(self._ctx, _capi.as_ptr(starts, ctypes.c_double), n, _capi.as_ptr(targets, ctypes.c_double),
                targets.shape[0], 1 if allow_contacts else 0, _capi.as_ptr(out, ctypes.c_double),
                _capi.as_ptr(collided, ctypes.c_uint8), _capi.as_ptr(micro, ctypes.c_uint32),
                _capi.as_ptr(resolver, ctypes.c_uint32), _capi.as_ptr(errors, ctypes.c_uint32))
        _capi.check(st, self._ctx, "fks_forward_simulate")
        return {"positions": out, "collided": collided.astype(bool), "microsteps": micro, "resolver_iterations": resolver,
                "error_flags": errors}

    def forward_simulate_path_arrays(self, robot: RobotDescription, start_positions, waypoints, allow_contacts: bool) -> dict:
        """A batch along a waypoint path in one launch (fks_forward_simulate_path): starts (n, W),
        waypoints (K, 1 or n, W) -- a (K, W) array is one shared waypoint per leg.  Returns
        [K, n, ...] arrays: leg k is what forward_simulate_arrays returns from leg k-1's positions
        toward waypoints[k] at call index get_call_index() + k, byte for byte; the call index
        advances by K."""
        self.set_robot(robot)
        W = robot.config_width
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        n = starts.shape[0]
        way, K, nt = _path_waypoints(waypoints, W, n)
        out = np.zeros((K, n, W), dtype=np.float64)
        collided = np.zeros((K, n), dtype=np.uint8)
        micro = np.zeros((K, n), dtype=np.uint32)
        resolver = np.zeros((K, n), dtype=np.uint32)
        errors = np.zeros((K, n), dtype=np.uint32)
        st = self._lib.fks_forward_simulate_path(
            self._ctx, _capi.as_ptr(starts, ctypes.c_double), n, _capi.as_ptr(way, ctypes.c_double), K, nt,
            1 if allow_contacts else 0, _capi.as_ptr(out, ctypes.c_double), _capi.as_ptr(collided, ctypes.c_uint8),
            _capi.as_ptr(micro, ctypes.c_uint32), _capi.as_ptr(resolver, ctypes.c_uint32), _capi.as_ptr(errors, ctypes.c_uint32))
        _capi.check(st, self._ctx, "fks_forward_simulate_path")
        return {"positions": out, "collided": collided.astype(bool), "microsteps": micro, "resolver_iterations": resolver,
                "error_flags": errors}

    def forward_simulate_policy_arrays(self, robot: RobotDescription, start_positions, table: "PolicyTable", max_legs: int,
                                       allow_contacts: bool) -> dict:
        """A batch rolled out under a policy table in one launch (fks_forward_simulate_policy): starts
        (n, W), K = max_legs.  Before every leg each particle selects the table entry nearest to where
        it is (policy_select); the entry's target is its next leg's, or it stops there (lost or
        arrived).  Returns the five [K, n, ...] arrays of a path plus "choice" uint32 [K + 1, n],
        "distance" [K + 1, n] and "legs_run" [n]; rows a particle does not run are defined
        (include/fks_capi.h).  The call index advances by K."""
        self.set_robot(robot)
        W = robot.config_width
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        n, K = starts.shape[0], int(max_legs)
        ctable, keep = table.to_c(W)
        out = np.zeros((K, n, W), dtype=np.float64)
        collided = np.zeros((K, n), dtype=np.uint8)
        micro = np.zeros((K, n), dtype=np.uint32)
        resolver = np.zeros((K, n), dtype=np.uint32)
        errors = np.zeros((K, n), dtype=np.uint32)
        choice = np.zeros((K + 1, n), dtype=np.uint32)
        distance = np.zeros((K + 1, n), dtype=np.float64)
        legs_run = np.zeros(n, dtype=np.uint32)
        st = self._lib.fks_forward_simulate_policy(
            self._ctx, _capi.as_ptr(starts, ctypes.c_double), n, ctypes.byref(ctable), K, 1 if allow_contacts else 0,
            _capi.as_ptr(out, ctypes.c_double), _capi.as_ptr(collided, ctypes.c_uint8), _capi.as_ptr(micro, ctypes.c_uint32),
            _capi.as_ptr(resolver, ctypes.c_uint32), _capi.as_ptr(errors, ctypes.c_uint32), _capi.as_ptr(choice, ctypes.c_uint32),
            _capi.as_ptr(distance, ctypes.c_double), _capi.as_ptr(legs_run, ctypes.c_uint32))
        del keep
        _capi.check(st, self._ctx, "fks_forward_simulate_policy")
        return {"positions": out, "collided": collided.astype(bool), "microsteps": micro, "resolver_iterations": resolver,
                "error_flags": errors, "choice": choice, "distance": distance, "legs_run": legs_run}

    def forward_simulate_jobs_arrays(self, robot: RobotDescription, jobs) -> list:
        """Many independent calls in one launch (fks_forward_simulate_jobs).  jobs: a sequence of
        (starts (n, W), targets (1 or n, W), allow_contacts).  Returns a list of the dicts
        forward_simulate_arrays returns: job j is what forward_simulate_arrays returns at call
        index get_call_index() + j, byte for byte; the call index advances by len(jobs)."""
        self.set_robot(robot)
        array, results, _keep = _host_jobs(jobs, robot.config_width)
        st = self._lib.fks_forward_simulate_jobs(self._ctx, array, len(results))
        _capi.check(st, self._ctx, "fks_forward_simulate_jobs")
        return [_job_result(r) for r in results]

    def forward_simulate_path_jobs_arrays(self, robot: RobotDescription, jobs) -> list:
        """Many independent waypoint paths in one launch (fks_forward_simulate_path_jobs).  jobs: a
        sequence of (starts (n, W), waypoints (K, 1 or n, W), allow_contacts); the jobs may differ
        in K.  Returns a list of the dicts forward_simulate_path_arrays returns ([K, n, ...]
        arrays): job j is what forward_simulate_path_arrays returns at call index
        get_call_index() + K_0 + ... + K_{j-1}, byte for byte; the call index advances by the sum
        of K."""
        self.set_robot(robot)
        array, results, _keep = _host_path_jobs(jobs, robot.config_width)
        st = self._lib.fks_forward_simulate_path_jobs(self._ctx, array, len(results))
        _capi.check(st, self._ctx, "fks_forward_simulate_path_jobs")
        return [_job_result(r) for r in results]

    def forward_simulate_mutable_arrays(self, robot: RobotDescription, start_positions, target_positions, allow_contacts: bool,
                                        controller_state) -> dict:
        """ForwardSimulateMutableRobot (SPCS:843-919) for a batch (fks_forward_simulate_mutable):
        each particle starts with its own PID state; controller_state is an (n, 2D) float64
        array (per dof the error integral, then per dof the last error), updated in place."""
        self.set_robot(robot)
        W, D = robot.config_width, robot.num_dofs
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        targets = np.ascontiguousarray(np.asarray(target_positions, dtype=np.float64).reshape(-1, W))
        n = starts.shape[0]
        if not (isinstance(controller_state, np.ndarray) and controller_state.dtype == np.float64 and
                controller_state.flags["C_CONTIGUOUS"] and controller_state.shape == (n, 2 * D)):
            raise ValueError("controller_state must be a C-contiguous float64 array of shape (n, 2 * num_dofs)")
        out = np.zeros((n, W), dtype=np.float64)
        collided = np.zeros(n, dtype=np.uint8)
        micro = np.zeros(n, dtype=np.uint32)
        resolver = np.zeros(n, dtype=np.uint32)
        errors = np.zeros(n, dtype=np.uint32)
        st = self._lib.fks_forward_simulate_mutable(
            self._ctx, _capi.as_ptr(starts, ctypes.c_double), n, _capi.as_ptr(targets, ctypes.c_double), targets.shape[0],
            1 if allow_contacts else 0, _capi.as_ptr(controller_state, ctypes.c_double), _capi.as_ptr(out, ctypes.c_double),
            _capi.as_ptr(collided, ctypes.c_uint8), _capi.as_ptr(micro, ctypes.c_uint32), _capi.as_ptr(resolver, ctypes.c_uint32),
            _capi.as_ptr(errors, ctypes.c_uint32))
        _capi.check(st, self._ctx, "fks_forward_simulate_mutable")
        return {"positions": out, "collided": collided.astype(bool), "microsteps": micro, "resolver_iterations": resolver,
                "error_flags": errors}

    def forward_simulate_robots(self, immutable_robot: RobotDescription, start_positions: Sequence, target_positions: Sequence,
                                allow_contacts: bool, display_fn: Optional[Callable] = None) -> List[SimulationResult]:
        """ForwardSimulateRobots (SPCS:788-804).  display_fn is accepted for interface
        parity; the batch path never draws (SPCS:801 passes enable_tracing=false)."""
        return self._results(immutable_robot, start_positions, target_positions, allow_contacts, reverse=False)

    def reverse_simulate_robots(self, immutable_robot: RobotDescription, start_positions: Sequence, target_positions: Sequence,
                                allow_contacts: bool, display_fn: Optional[Callable] = None) -> List[SimulationResult]:
        """ReverseSimulateRobots (SPCS:806-822) == forward simulation (SPCS:838-841)."""
        return self._results(immutable_robot, start_positions, target_positions, allow_contacts, reverse=True)

    def forward_simulate_robot(self, immutable_robot: RobotDescription, start_position, target_position,
                               allow_contacts: bool) -> SimulationResult:
        """ForwardSimulateRobot (SPCS:824-829) as a batch of one."""
        return self._results(immutable_robot, [start_position], [target_position], allow_contacts, reverse=False)[0]

    def forward_simulate_traced(self, robot: RobotDescription, start_positions, target_positions, allow_contacts: bool,
                                step_capacity: Optional[int] = None, config_capacity: int = 4096):
        """ForwardSimulateRobot with ``enable_tracing = true`` (SPCS:824-829) for a batch:
        returns (result dict as forward_simulate_arrays, TraceBuffers).  Capacities are
        per particle; records past them are counted, not stored (``truncated``)."""
        self.set_robot(robot)
        W, D = robot.config_width, robot.num_dofs
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        targets = np.ascontiguousarray(np.asarray(target_positions, dtype=np.float64).reshape(-1, W))
        n = starts.shape[0]
        if n > 0 and targets.shape[0] not in (1, n):
            raise ValueError("target_positions must hold 1 or len(start_positions) configurations (SPCS:792)")
        if step_capacity is None:
            step_capacity = max(1, int(self.solver_config.forward_simulation_time * self.simulation_controller_frequency))
        buf = TraceBuffers(n, D, W, step_capacity, config_capacity)
        tr = buf.to_c()
        out = np.zeros((n, W), dtype=np.float64)
        collided = np.zeros(n, dtype=np.uint8)
        micro = np.zeros(n, dtype=np.uint32)
        resolver = np.zeros(n, dtype=np.uint32)
        errors = np.zeros(n, dtype=np.uint32)
        st = self._lib.fks_forward_simulate_traced(
            self._ctx, _capi.as_ptr(starts, ctypes.c_double), n, _capi.as_ptr(targets, ctypes.c_double), targets.shape[0],
            1 if allow_contacts else 0, _capi.as_ptr(out, ctypes.c_double), _capi.as_ptr(collided, ctypes.c_uint8),
            _capi.as_ptr(micro, ctypes.c_uint32), _capi.as_ptr(resolver, ctypes.c_uint32), _capi.as_ptr(errors, ctypes.c_uint32),
            ctypes.byref(tr))
        _capi.check(st, self._ctx, "fks_forward_simulate_traced")
        return ({"positions": out, "collided": collided.astype(bool), "microsteps": micro, "resolver_iterations": resolver,
                 "error_flags": errors}, buf)

    def forward_simulate_traced_mutable(self, robot: RobotDescription, start_positions, target_positions, allow_contacts: bool,
                                        controller_state, step_capacity: Optional[int] = None, config_capacity: int = 4096):
        """ForwardSimulateMutableRobot with ``enable_tracing = true`` (SPCS:843-919) for a batch
        (fks_forward_simulate_traced_mutable): forward_simulate_mutable_arrays' controller state,
        an (n, 2D) float64 array updated in place, plus forward_simulate_traced's trace.
        Returns (result dict, TraceBuffers)."""
        self.set_robot(robot)
        W, D = robot.config_width, robot.num_dofs
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        targets = np.ascontiguousarray(np.asarray(target_positions, dtype=np.float64).reshape(-1, W))
        n = starts.shape[0]
        if n > 0 and targets.shape[0] not in (1, n):
            raise ValueError("target_positions must hold 1 or len(start_positions) configurations (SPCS:792)")
        if not (isinstance(controller_state, np.ndarray) and controller_state.dtype == np.float64 and
                controller_state.flags["C_CONTIGUOUS"] and controller_state.shape == (n, 2 * D)):
            raise ValueError("controller_state must be a C-contiguous float64 array of shape (n, 2 * num_dofs)")
        if step_capacity is None:
            step_capacity = max(1, int(self.solver_config.forward_simulation_time * self.simulation_controller_frequency))
        buf = TraceBuffers(n, D, W, step_capacity, config_capacity)
        tr = buf.to_c()
        out = np.zeros((n, W), dtype=np.float64)
        collided = np.zeros(n, dtype=np.uint8)
        micro = np.zeros(n, dtype=np.uint32)
        resolver = np.zeros(n, dtype=np.uint32)
        errors = np.zeros(n, dtype=np.uint32)
        st = self._lib.fks_forward_simulate_traced_mutable(
            self._ctx, _capi.as_ptr(starts, ctypes.c_double), n, _capi.as_ptr(targets, ctypes.c_double), targets.shape[0],
            1 if allow_contacts else 0, _capi.as_ptr(controller_state, ctypes.c_double), _capi.as_ptr(out, ctypes.c_double),
            _capi.as_ptr(collided, ctypes.c_uint8), _capi.as_ptr(micro, ctypes.c_uint32), _capi.as_ptr(resolver, ctypes.c_uint32),
            _capi.as_ptr(errors, ctypes.c_uint32), ctypes.byref(tr))
        _capi.check(st, self._ctx, "fks_forward_simulate_traced_mutable")
        return ({"positions": out, "collided": collided.astype(bool), "microsteps": micro, "resolver_iterations": resolver,
                 "error_flags": errors}, buf)

    def forward_simulate_robot_traced(self, immutable_robot: RobotDescription, start_position, target_position,
                                      allow_contacts: bool):
        """ForwardSimulateRobot(..., trace, enable_tracing=true, ...) (SPCS:824-829):
        (SimulationResult, ForwardSimulationStepTrace)."""
        W = immutable_robot.config_width
        r, buf = self.forward_simulate_traced(immutable_robot, [start_position], [target_position], allow_contacts)
        tgt = np.asarray(target_position, dtype=np.float64).reshape(W)
        res = SimulationResult(r["positions"][0].copy(), tgt.copy(), bool(r["collided"][0]), True, int(r["microsteps"][0]),
                               int(r["resolver_iterations"][0]), int(r["error_flags"][0]))
        return res, buf.particle(0)

    def _results(self, robot, starts, targets, allow_contacts, reverse):
        W = robot.config_width
        tarr = np.asarray(targets, dtype=np.float64).reshape(-1, W)
        r = self.forward_simulate_arrays(robot, starts, tarr, allow_contacts, reverse=reverse)
        n = r["positions"].shape[0]
        out = []
        for i in range(n):
            tgt = tarr[i] if tarr.shape[0] == n else tarr[0]
            out.append(SimulationResult(r["positions"][i].copy(), tgt.copy(), bool(r["collided"][i]), True,
                                        int(r["microsteps"][i]), int(r["resolver_iterations"][i]), int(r["error_flags"][i])))
        return out

    def check_config_collisions(self, robot: RobotDescription, configs, inflation_ratio: float = 0.0) -> dict:
        """Batched CheckConfigCollision (SPCS:1398-1416): configs (n, W) -> collided[n]
        (bool) and error_flags[n]."""
        self.set_robot(robot)
        W = robot.config_width
        arr = np.ascontiguousarray(np.asarray(configs, dtype=np.float64).reshape(-1, W))
        n = arr.shape[0]
        collided = np.zeros(n, dtype=np.uint8)
        errors = np.zeros(n, dtype=np.uint32)
        st = self._lib.fks_check_config_collision(self._ctx, _capi.as_ptr(arr, ctypes.c_double), n, float(inflation_ratio),
                                                  _capi.as_ptr(collided, ctypes.c_uint8), _capi.as_ptr(errors, ctypes.c_uint32))
        _capi.check(st, self._ctx, "fks_check_config_collision")
        return {"collided": collided.astype(bool), "error_flags": errors}

    def check_config_collision(self, immutable_robot: RobotDescription, config, inflation_ratio: float) -> bool:
        """CheckConfigCollision (SPCS:1398-1416) for one configuration."""
        return bool(self.check_config_collisions(immutable_robot, [config], inflation_ratio)["collided"][0])

    def check_config_collisions_device(self, robot: RobotDescription, d_configs, n: int, inflation_ratio: float,
                                       d_out_collided, d_out_error_flags=0, stream=0, synchronize=False):
        """fks_check_config_collision_device: device pointers (int) on `stream`."""
        self.set_robot(robot)
        st = self._lib.fks_check_config_collision_device(
            self._ctx, ctypes.c_void_p(d_configs), n, float(inflation_ratio), ctypes.c_void_p(d_out_collided),
            ctypes.c_void_p(d_out_error_flags or None), ctypes.c_void_p(stream or None), 1 if synchronize else 0)
        _capi.check(st, self._ctx, "fks_check_config_collision_device")

    def last_check_counters(self) -> dict:
        c = _capi.CallCounters()
        _capi.check(self._lib.fks_get_last_check_counters(self._ctx, ctypes.byref(c)), self._ctx, "counters")
        return c.as_dict()

    # ---- kinematics helpers of the interface (fks_kinematics) ----
    def _kinematics(self, robot: RobotDescription, mode: int, configs, inputs=None) -> np.ndarray:
        self.set_robot(robot)
        W = robot.config_width
        cfg = np.ascontiguousarray(np.asarray(configs, dtype=np.float64).reshape(-1, W))
        n = cfg.shape[0]
        links, points, dofs = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _capi.check(self._lib.fks_robot_sizes(self._ctx, ctypes.byref(links), ctypes.byref(points), ctypes.byref(dofs), None),
                    self._ctx, "fks_robot_sizes")
        shape = {_capi.KIN_LINK_TRANSFORMS: (n, links.value, 3, 4), _capi.KIN_POINTS: (n, points.value, 3),
                 _capi.KIN_APPLY_CONTROL_INPUT: (n, W)}[mode]
        out = np.zeros(shape, dtype=np.float64)
        u = None
        if mode == _capi.KIN_APPLY_CONTROL_INPUT:
            u = np.ascontiguousarray(np.asarray(inputs, dtype=np.float64).reshape(n, dofs.value))
        st = self._lib.fks_kinematics(self._ctx, mode, _capi.as_ptr(cfg, ctypes.c_double), n,
                                      _capi.as_ptr(u, ctypes.c_double) if u is not None else None,
                                      _capi.as_ptr(out, ctypes.c_double))
        _capi.check(st, self._ctx, "fks_kinematics")
        return out

    def link_transforms(self, robot: RobotDescription, configs) -> np.ndarray:
        """GetLinkTransform of every link after SetPosition: (n, links, 3, 4)."""
        return self._kinematics(robot, _capi.KIN_LINK_TRANSFORMS, configs)

    def world_points(self, robot: RobotDescription, configs) -> np.ndarray:
        """Every link point in the world frame, geometry order: (n, points, 3)."""
        return self._kinematics(robot, _capi.KIN_POINTS, configs)

    def apply_control_input(self, robot: RobotDescription, configs, control_inputs) -> np.ndarray:
        """SetPosition + clean ApplyControlInput (TNUVA:538-566): (n, W)."""
        return self._kinematics(robot, _capi.KIN_APPLY_CONTROL_INPUT, configs, control_inputs)

    def get_frame(self) -> str:
        """GetFrame (SPCS:517-520)."""
        return self.environment.frame

    def get_resolution(self) -> float:
        return float(self.environment.resolution)

    def get_random_generator(self) -> np.random.Generator:
        """GetRandomGenerator (SPCS:473-481) for the caller's own sampling.  The
        simulation's actuation noise does not come from it: that is the counter RNG keyed
        by (seed, call index, particle, step, microstep, dof), DESIGN.md §2.1."""
        if getattr(self, "_host_rng", None) is None:
            self._host_rng = np.random.default_rng(self.prng_seed)
        return self._host_rng

    def get_3d_point_for_config(self, immutable_robot: RobotDescription, config) -> np.ndarray:
        """Get3dPointForConfig (SPCS:776-786): the origin of the last geometry's link."""
        T = self.link_transforms(immutable_robot, [config])[0, immutable_robot.geometry_link[-1]]
        return np.array([T[0, 3], T[1, 3], T[2, 3], 1.0])

    def make_configuration_display_rep(self, immutable_robot: RobotDescription, configuration, color,
                                       starting_index: int, config_marker_ns: str) -> List[dict]:
        """MakeConfigurationDisplayRep for POINTS geometries (SPCS:634-688): one SPHERE_LIST
        marker of every link point, black where the link-frame point is the zero vector."""
        pts = self.world_points(immutable_robot, [configuration])[0]
        res = self.get_resolution()
        m = _marker(config_marker_ns, starting_index, "SPHERE_LIST", self.get_frame(), (res, res, res), color)
        m["points"] = pts.tolist()
        link_pts = immutable_robot.points
        black = [0.0, 0.0, 0.0, 1.0]
        m["colors"] = [black if float(np.linalg.norm(p)) == 0.0 else list(color) for p in link_pts]
        return [m]

    def make_control_input_display_rep(self, immutable_robot: RobotDescription, configuration, control_input, color,
                                       starting_index: int, control_input_marker_ns: str) -> List[dict]:
        """MakeControlInputDisplayRep (SPCS:719-774): a LINE_LIST from every point at
        `configuration` to the same point after the clean control input."""
        after = self.apply_control_input(immutable_robot, [configuration], [control_input])
        pts = self.world_points(immutable_robot, np.concatenate([np.asarray(configuration, dtype=np.float64).reshape(1, -1),
                                                                 after], axis=0))
        res = self.get_resolution() * 0.5
        m = _marker(control_input_marker_ns, starting_index, "LINE_LIST", self.get_frame(), (res, res, res), color)
        m["points"] = np.stack([pts[0], pts[1]], axis=1).reshape(-1, 3).tolist()
        m["colors"] = [list(color)] * (2 * pts.shape[1])
        return [m]

    def make_environment_display_rep(self) -> List[dict]:
        """MakeEnvironmentDisplayRep (SPCS:559-586), reduced to what this repository holds:
        the filled cells of the collision grid ("sim_environment") and the SDF cells
        colored by sign ("sim_environment_sdf").  sdf_tools' connected-component and
        convex-segment exports have no counterpart here."""
        env = self.environment.download() if isinstance(self.environment, DeviceEnvironment) else self.environment
        g = env.geometry
        n = tuple(int(v) for v in g.num_cells)
        o = np.asarray(g.origin, dtype=np.float64).reshape(3, 4)
        idx = np.stack(np.unravel_index(np.arange(int(np.prod(n))), n), axis=1).astype(np.float64)
        centers = (idx + 0.5) * g.resolution @ o[:, :3].T + o[:, 3]
        res = float(g.resolution)
        markers = []
        occ = env.occupancy if env.occupancy is not None else (env.sdf < 0).astype(np.uint8)
        m = _marker("sim_environment", 1, "CUBE_LIST", self.get_frame(), (res, res, res), [1.0, 0.0, 0.0, 1.0])
        m["points"] = centers[occ.astype(bool)].tolist()
        markers.append(m)
        s = _marker("sim_environment_sdf", 1, "CUBE_LIST", self.get_frame(), (res, res, res), [1.0, 1.0, 1.0, 1.0])
        s["points"] = centers.tolist()
        s["colors"] = [[1.0, 0.0, 0.0, 1.0] if v < 0 else [0.0, 0.0, 1.0, 1.0] for v in env.sdf]
        markers.append(s)
        return markers

    def forward_simulate_device(self, robot: RobotDescription, d_starts, n: int, d_targets, num_targets: int,
                                first_particle_id: int, allow_contacts: bool, d_out_positions, d_out_collided=0,
                                d_out_microsteps=0, d_out_resolver_iterations=0, d_out_error_flags=0, stream=0,
                                synchronize=False):
        """fks_forward_simulate_device: every buffer is a device pointer (int), e.g.
        torch_tensor.data_ptr(); `stream` a hipStream_t handle (int)."""
        self.set_robot(robot)
        st = self._lib.fks_forward_simulate_device(
            self._ctx, ctypes.c_void_p(d_starts), n, ctypes.c_void_p(d_targets), num_targets, first_particle_id,
            1 if allow_contacts else 0, ctypes.c_void_p(d_out_positions), ctypes.c_void_p(d_out_collided or None),
            ctypes.c_void_p(d_out_microsteps or None), ctypes.c_void_p(d_out_resolver_iterations or None),
            ctypes.c_void_p(d_out_error_flags or None), ctypes.c_void_p(stream or None), 1 if synchronize else 0)
        _capi.check(st, self._ctx, "fks_forward_simulate_device")

    def forward_simulate_path_device(self, robot: RobotDescription, d_starts, n: int, d_waypoints, num_legs: int, num_targets: int,
                                     first_particle_id: int, allow_contacts: bool, d_out_positions, d_out_collided=0,
                                     d_out_microsteps=0, d_out_resolver_iterations=0, d_out_error_flags=0, stream=0,
                                     synchronize=False):
        """fks_forward_simulate_path_device: device pointers (int) as in forward_simulate_device;
        d_waypoints [num_legs][num_targets][W], the outputs leg-major ([num_legs][n]...)."""
        self.set_robot(robot)
        st = self._lib.fks_forward_simulate_path_device(
            self._ctx, ctypes.c_void_p(d_starts), n, ctypes.c_void_p(d_waypoints), num_legs, num_targets, first_particle_id,
            1 if allow_contacts else 0, ctypes.c_void_p(d_out_positions), ctypes.c_void_p(d_out_collided or None),
            ctypes.c_void_p(d_out_microsteps or None), ctypes.c_void_p(d_out_resolver_iterations or None),
            ctypes.c_void_p(d_out_error_flags or None), ctypes.c_void_p(stream or None), 1 if synchronize else 0)
        _capi.check(st, self._ctx, "fks_forward_simulate_path_device")

    def forward_simulate_policy_device(self, robot: RobotDescription, d_starts, n: int, d_keys, d_targets, d_flags, num_entries: int,
                                       terminal_distance: float, max_distance: float, max_legs: int, first_particle_id: int,
                                       allow_contacts: bool, d_out_positions, d_out_choice, d_out_distance=0, d_out_legs_run=0,
                                       d_out_collided=0, d_out_microsteps=0, d_out_resolver_iterations=0, d_out_error_flags=0,
                                       stream=0, synchronize=False):
        """fks_forward_simulate_policy_device: device pointers (int) as in forward_simulate_device, the
        table's three included (d_flags may be 0); the five simulation outputs leg-major
        ([max_legs][n]...), d_out_choice uint32 and d_out_distance double [max_legs + 1][n],
        d_out_legs_run uint32 [n]."""
        self.set_robot(robot)
        table = _capi.PolicyTable(d_keys or None, d_targets or None, d_flags or None, int(num_entries), float(terminal_distance),
                                  float(max_distance))
        st = self._lib.fks_forward_simulate_policy_device(
            self._ctx, ctypes.c_void_p(d_starts or None), n, ctypes.byref(table), int(max_legs), first_particle_id,
            1 if allow_contacts else 0, ctypes.c_void_p(d_out_positions or None), ctypes.c_void_p(d_out_collided or None),
            ctypes.c_void_p(d_out_microsteps or None), ctypes.c_void_p(d_out_resolver_iterations or None),
            ctypes.c_void_p(d_out_error_flags or None), ctypes.c_void_p(d_out_choice or None),
            ctypes.c_void_p(d_out_distance or None), ctypes.c_void_p(d_out_legs_run or None), ctypes.c_void_p(stream or None),
            1 if synchronize else 0)
        _capi.check(st, self._ctx, "fks_forward_simulate_policy_device")

    def forward_simulate_jobs_device(self, robot: RobotDescription, jobs, stream=0, synchronize=False):
        """fks_forward_simulate_jobs_device: jobs is a sequence of dicts with the fields of fks_job
        (d_starts, n, d_targets, num_targets, allow_contacts, d_out_positions and optionally
        first_particle_id, d_out_collided, d_out_microsteps, d_out_resolver_iterations,
        d_out_error_flags), every buffer a device pointer (int) as in forward_simulate_device."""
        self.set_robot(robot)
        array = (_capi.Job * max(len(jobs), 1))()
        for j, job in enumerate(jobs):
            array[j] = _capi.Job(
                job["d_starts"] or None, int(job["n"]), job["d_targets"] or None, int(job["num_targets"]),
                int(job.get("first_particle_id", 0)), 1 if job["allow_contacts"] else 0, 0, job["d_out_positions"] or None,
                job.get("d_out_collided") or None, job.get("d_out_microsteps") or None,
                job.get("d_out_resolver_iterations") or None, job.get("d_out_error_flags") or None)
        st = self._lib.fks_forward_simulate_jobs_device(self._ctx, array, len(jobs), ctypes.c_void_p(stream or None),
                                                        1 if synchronize else 0)
        _capi.check(st, self._ctx, "fks_forward_simulate_jobs_device")

    def forward_simulate_path_jobs_device(self, robot: RobotDescription, jobs, stream=0, synchronize=False):
        """fks_forward_simulate_path_jobs_device: jobs is a sequence of dicts with the fields of
        fks_path_job (d_starts, n, d_waypoints, num_legs, num_targets, allow_contacts,
        d_out_positions and optionally first_particle_id, d_out_collided, d_out_microsteps,
        d_out_resolver_iterations, d_out_error_flags), every buffer a device pointer (int) as in
        forward_simulate_device; the outputs are leg-major with the job's own n as leg stride."""
        self.set_robot(robot)
        array = (_capi.PathJob * max(len(jobs), 1))()
        for j, job in enumerate(jobs):
            array[j] = _capi.PathJob(
                job["d_starts"] or None, int(job["n"]), job["d_waypoints"] or None, int(job["num_legs"]), int(job["num_targets"]),
                int(job.get("first_particle_id", 0)), 1 if job["allow_contacts"] else 0, 0, job["d_out_positions"] or None,
                job.get("d_out_collided") or None, job.get("d_out_microsteps") or None,
                job.get("d_out_resolver_iterations") or None, job.get("d_out_error_flags") or None)
        st = self._lib.fks_forward_simulate_path_jobs_device(self._ctx, array, len(jobs), ctypes.c_void_p(stream or None),
                                                             1 if synchronize else 0)
        _capi.check(st, self._ctx, "fks_forward_simulate_path_jobs_device")

    def cluster_outcomes(self, robot: RobotDescription, groups, threshold: float, distances: bool = False) -> dict:
        """fks_cluster_configs_ctx: the complete-link clusters of each group of configurations under
        `threshold` by the robot's configuration distance, in one launch (include/fks_capi.h).
        groups is a sequence of (n_g, W) arrays.  Returns per group "labels" (uint32 [n_g]), "counts"
        uint32 [G] and, with distances=True, "distances" (a list of (n_g, n_g) arrays)."""
        self.set_robot(robot)
        configs, begin = _cluster_groups(groups, robot.config_width)
        out = _cluster_outputs(begin, True, distances)
        st = self._lib.fks_cluster_configs_ctx(self._ctx, _cluster_ptr(configs, ctypes.c_double), _capi.as_ptr(begin, ctypes.c_uint64),
                                               len(begin) - 1, float(threshold), _cluster_ptr(out[0], ctypes.c_double),
                                               _cluster_ptr(out[1], ctypes.c_uint32), _cluster_ptr(out[2], ctypes.c_uint32))
        _capi.check(st, self._ctx, "fks_cluster_configs_ctx")
        return _cluster_result(begin, *out)

    def cluster_outcomes_device(self, robot: RobotDescription, d_configs, group_begin, threshold: float, d_out_distances=0,
                                d_out_labels=0, d_out_num_clusters=0, stream=0, synchronize=False):
        """fks_cluster_configs_device: d_configs is a device pointer (int), e.g. the data_ptr() of
        the tensor a jobs call wrote its positions to; group_begin the G + 1 ascending offsets (in
        configurations, a host sequence); the three outputs device pointers (each may be 0, not
        all): doubles [sum of n_g^2], uint32 [N] and uint32 [G]."""
        self.set_robot(robot)
        begin = np.ascontiguousarray(np.asarray(group_begin, dtype=np.uint64).reshape(-1))
        if begin.size == 0:
            begin = np.zeros(1, dtype=np.uint64)
        st = self._lib.fks_cluster_configs_device(
            self._ctx, ctypes.c_void_p(d_configs or None), _capi.as_ptr(begin, ctypes.c_uint64), begin.size - 1, float(threshold),
            ctypes.c_void_p(d_out_distances or None), ctypes.c_void_p(d_out_labels or None),
            ctypes.c_void_p(d_out_num_clusters or None), ctypes.c_void_p(stream or None), 1 if synchronize else 0)
        _capi.check(st, self._ctx, "fks_cluster_configs_device")

    def summarize_clusters(self, robot: RobotDescription, groups, labels, targets=None, reached_distance: float = 0.0,
                           outputs=None) -> dict:
        """fks_summarize_clusters_ctx: every cluster of every group as a child state, in one launch
        (include/fks_capi.h).  groups and labels are sequences of (n_g, W) and (n_g,) arrays, as
        cluster_outcomes takes and returns them; targets (G, W) or None.  Returns the arrays named in
        `outputs` (None: all of SUMMARY_OUTPUTS, "reached" only with targets), each with N rows, and
        "group_begin"."""
        self.set_robot(robot)
        call = _SummaryCall(robot, groups, labels, targets, outputs)
        st = self._lib.fks_summarize_clusters_ctx(self._ctx, *call.inputs(), float(reached_distance), ctypes.byref(call.struct))
        _capi.check(st, self._ctx, "fks_summarize_clusters_ctx")
        return call.result()

    def summarize_clusters_device(self, robot: RobotDescription, d_configs, group_begin, d_labels, d_targets=0,
                                  reached_distance: float = 0.0, d_out=None, stream=0, synchronize=False):
        """fks_summarize_clusters_device: d_configs and d_labels are device pointers (int), e.g. the
        buffers a jobs call and a clustering call wrote; group_begin the G + 1 ascending offsets (a
        host sequence); d_targets a device pointer to (G, W) doubles or 0; d_out a dict of device
        pointers by output name (SUMMARY_OUTPUTS; absent or 0: not asked for), each of N rows."""
        self.set_robot(robot)
        begin = np.ascontiguousarray(np.asarray(group_begin, dtype=np.uint64).reshape(-1))
        if begin.size == 0:
            begin = np.zeros(1, dtype=np.uint64)
        d_out = d_out or {}
        unknown = set(d_out) - set(SUMMARY_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown summary outputs {sorted(unknown)}")
        struct = _capi.ClusterSummary(**{name: (d_out.get(name) or None) for name in SUMMARY_OUTPUTS})
        st = self._lib.fks_summarize_clusters_device(
            self._ctx, ctypes.c_void_p(d_configs or None), _capi.as_ptr(begin, ctypes.c_uint64), begin.size - 1,
            ctypes.c_void_p(d_labels or None), ctypes.c_void_p(d_targets or None), float(reached_distance), ctypes.byref(struct),
            ctypes.c_void_p(stream or None), 1 if synchronize else 0)
        _capi.check(st, self._ctx, "fks_summarize_clusters_device")

    def select_states(self, robot: RobotDescription, keys, queries, num_particles: int = 0, draw_seed: int = 0, weights=None,
                      count=None, begin=None, members=None, outputs=None) -> dict:
        """fks_select_states_ctx: for every query (J, W) the nearest of the states `keys` (S, W) under
        the per-state `weights`, and the chosen state's members drawn into num_particles starts
        (include/fks_capi.h).  Returns the arrays named in `outputs` (None: choice and distance, and
        starts and source when num_particles > 0 and count, begin, members are given)."""
        self.set_robot(robot)
        call = _SelectCall(robot, keys, queries, num_particles, weights, count, begin, members, outputs)
        st = self._lib.fks_select_states_ctx(self._ctx, ctypes.byref(call.table), *call.inputs(), ctypes.c_uint64(int(draw_seed)),
                                             ctypes.byref(call.struct))
        _capi.check(st, self._ctx, "fks_select_states_ctx")
        return call.result()

    def select_states_device(self, robot: RobotDescription, d_table: dict, num_states: int, d_queries, num_queries: int,
                             num_particles: int, draw_seed: int, d_out: dict, num_member_rows: int = 0, stream=0, synchronize=False):
        """fks_select_states_device: d_table holds device pointers (int) by name (keys, weights, count,
        begin, members; absent or 0: NULL), e.g. the buffers successive summaries appended to; d_queries a
        device pointer to (J, W) doubles; d_out device pointers by output name (SELECT_OUTPUTS).
        `starts` is fit to be the next jobs call's starts by device pointer."""
        self.set_robot(robot)
        unknown = (set(d_table) - set(SELECT_TABLE)) | (set(d_out) - set(SELECT_OUTPUTS))
        if unknown:
            raise ValueError(f"unknown selection arrays {sorted(unknown)}")
        table = _capi.StateTable(num_states=int(num_states), num_member_rows=int(num_member_rows),
                                 **{name: (d_table.get(name) or None) for name in SELECT_TABLE})
        struct = _capi.StateSelection(**{name: (d_out.get(name) or None) for name in SELECT_OUTPUTS})
        st = self._lib.fks_select_states_device(
            self._ctx, ctypes.byref(table), ctypes.c_void_p(d_queries or None), int(num_queries), int(num_particles),
            ctypes.c_uint64(int(draw_seed)), ctypes.byref(struct), ctypes.c_void_p(stream or None), 1 if synchronize else 0)
        _capi.check(st, self._ctx, "fks_select_states_device")


# the arrays of a selection call, in the order of fks_state_table and fks_state_selection
SELECT_TABLE = ("keys", "weights", "count", "begin", "members")
SELECT_OUTPUTS = ("choice", "distance", "starts", "source")


class _SelectCall:
    """the host arrays of one selection call: the table, the queries, the outputs asked for and the structs that name them"""

    def __init__(self, robot, keys, queries, num_particles, weights, count, begin, members, outputs):
        W = robot.config_width
        f64 = lambda a, shape: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
        u32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
        self.keys, self.queries = f64(keys, (-1, W)), f64(queries, (-1, W))
        self.weights, self.members = f64(weights, (-1,)), f64(members, (-1, W))
        self.count, self.begin = u32(count), u32(begin)
        S, J, P = self.keys.shape[0], self.queries.shape[0], int(num_particles)
        for name, a in (("weights", self.weights), ("count", self.count), ("begin", self.begin)):
            if a is not None and a.size != S:
                raise ValueError(f"{name} must hold one entry per state")
        self.J, self.P = J, P
        if outputs is None:
            drawn = P > 0 and all(a is not None for a in (count, begin, members))
            outputs = ("choice", "distance") + (("starts", "source") if drawn else ())
        unknown = set(outputs) - set(SELECT_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown selection outputs {sorted(unknown)}")
        shapes = {"choice": ((J,), np.uint32), "distance": ((J,), np.float64), "starts": ((J, P, W), np.float64),
                  "source": ((J, P), np.uint32)}
        names = [n for n in SELECT_OUTPUTS if n in outputs]
        # one spare element keeps a pointer non-NULL for an empty array
        self.flat = {n: np.zeros(int(np.prod(shapes[n][0])) + 1, dtype=shapes[n][1]) for n in names}
        self.shapes = {n: shapes[n][0] for n in names}
        self.struct = _capi.StateSelection(**{n: self.flat[n].ctypes.data for n in names})
        ptr = lambda a: None if a is None else a.ctypes.data
        # (an empty members array is still a pool, of no rows: the spare keeps it non-NULL)
        self._spare = np.zeros(1, dtype=np.float64)
        members_ptr = None if self.members is None else (self.members.ctypes.data if self.members.size else self._spare.ctypes.data)
        self.table = _capi.StateTable(keys=ptr(self.keys) if S else None, weights=ptr(self.weights), count=ptr(self.count),
                                      begin=ptr(self.begin), members=members_ptr, num_states=S,
                                      num_member_rows=0 if self.members is None else self.members.shape[0])

    def inputs(self):
        return (_cluster_ptr(self.queries, ctypes.c_double), self.J, self.P)

    def result(self) -> dict:
        return {n: a[:-1].reshape(self.shapes[n]).copy() for n, a in self.flat.items()}


def select_states_host(robot: RobotDescription, keys, queries, num_particles: int = 0, draw_seed: int = 0, weights=None, count=None,
                       begin=None, members=None, outputs=None) -> dict:
    """fks_select_states: the host twin of Simulator.select_states, with the kernels' arithmetic and
    without a context or a GPU; the same result byte for byte."""
    call = _SelectCall(robot, keys, queries, num_particles, weights, count, begin, members, outputs)
    desc, keep = robot.to_c()
    st = _capi.lib().fks_select_states(ctypes.byref(desc), ctypes.byref(call.table), *call.inputs(), ctypes.c_uint64(int(draw_seed)),
                                       ctypes.byref(call.struct))
    del keep
    _capi.check(st, None, "fks_select_states")
    return call.result()


def select_states_plan(num_queries: int, num_states: int, compute_units: int) -> dict:
    """fks_select_states_plan: the decomposition of a device call (queries per workgroup, states per
    chunk, chunks per query, workgroups of the search)."""
    out = (ctypes.c_uint64 * 4)()
    _capi.check(_capi.lib().fks_select_states_plan(int(num_queries), int(num_states), int(compute_units), out), None,
                "fks_select_states_plan")
    return {"tile": int(out[0]), "chunk_states": int(out[1]), "chunks": int(out[2]), "groups": int(out[3])}



class _SummaryCall:
    """the host arrays of one summary call: inputs, the outputs asked for and the struct that names them"""

    def __init__(self, robot, groups, labels, targets, outputs):
        W = robot.config_width
        self.configs, self.begin = _cluster_groups(groups, W)
        N, G = int(self.begin[-1]), len(self.begin) - 1
        lab = [np.asarray(l, dtype=np.uint32).reshape(-1) for l in labels]
        if [l.size for l in lab] != [int(v) for v in np.diff(self.begin)]:
            raise ValueError("labels must hold one array per group, of the group's length")
        self.labels = np.ascontiguousarray(np.concatenate(lab)) if lab else np.zeros(0, dtype=np.uint32)
        self.targets = None if targets is None else np.ascontiguousarray(np.asarray(targets, dtype=np.float64).reshape(G, W))
        Wv = W if robot.robot_type == _capi.ROBOT_LINKED else (3 if robot.robot_type == _capi.ROBOT_SE2 else 6)
        shapes = {"order": ((N,), np.uint32), "members": ((N, W), np.float64), "count": ((N,), np.uint32), "begin": ((N,), np.uint32),
                  "expectation": ((N, W), np.float64), "variances": ((N, Wv), np.float64), "variance": ((N,), np.float64),
                  "reached": ((N,), np.uint32)}
        if outputs is None:
            outputs = [n for n in SUMMARY_OUTPUTS if n != "reached" or self.targets is not None]
        unknown = set(outputs) - set(shapes)
        if unknown:
            raise ValueError(f"unknown summary outputs {sorted(unknown)}")
        names = [n for n in SUMMARY_OUTPUTS if n in outputs]
        # one spare element keeps a pointer non-NULL for N == 0
        self.flat = {n: np.zeros(int(np.prod(shapes[n][0])) + 1, dtype=shapes[n][1]) for n in names}
        self.shapes = {n: shapes[n][0] for n in names}
        self.struct = _capi.ClusterSummary(**{n: self.flat[n].ctypes.data for n in names})

    def inputs(self):
        return (_cluster_ptr(self.configs, ctypes.c_double), _capi.as_ptr(self.begin, ctypes.c_uint64), len(self.begin) - 1,
                _cluster_ptr(self.labels, ctypes.c_uint32), _cluster_ptr(self.targets, ctypes.c_double))

    def result(self) -> dict:
        out = {n: a[:-1].reshape(self.shapes[n]).copy() for n, a in self.flat.items()}
        out["group_begin"] = self.begin.copy()
        return out


def summarize_clusters_host(robot: RobotDescription, groups, labels, targets=None, reached_distance: float = 0.0,
                            outputs=None) -> dict:
    """fks_summarize_clusters: the host twin of Simulator.summarize_clusters, with the kernels'
    arithmetic and without a context or a GPU; the same result byte for byte."""
    call = _SummaryCall(robot, groups, labels, targets, outputs)
    desc, keep = robot.to_c()
    st = _capi.lib().fks_summarize_clusters(ctypes.byref(desc), *call.inputs(), float(reached_distance), ctypes.byref(call.struct))
    del keep
    _capi.check(st, None, "fks_summarize_clusters")
    return call.result()


def _cluster_groups(groups, W: int):
    """configs (N, W) and group_begin uint64 [G + 1] of a sequence of (n_g, W) arrays"""
    arrays = [np.asarray(g, dtype=np.float64).reshape(-1, W) for g in groups]
    begin = np.zeros(len(arrays) + 1, dtype=np.uint64)
    if arrays:
        begin[1:] = np.cumsum([a.shape[0] for a in arrays], dtype=np.uint64)
    configs = np.ascontiguousarray(np.concatenate(arrays, axis=0)) if arrays else np.zeros((0, W), dtype=np.float64)
    return configs, begin


def _cluster_ptr(array, ctype):
    return _capi.as_ptr(array, ctype) if array is not None and array.size else None


def _cluster_outputs(begin, labels: bool, distances: bool):
    sizes = np.diff(begin).astype(np.uint64)
    mats = np.zeros(max(int((sizes * sizes).sum()), 1), dtype=np.float64) if distances else None
    lab = np.zeros(max(int(begin[-1]), 1), dtype=np.uint32) if labels else None
    cnt = np.zeros(max(len(begin) - 1, 1), dtype=np.uint32) if labels else None
    return mats, lab, cnt


def _cluster_result(begin, mats, lab, cnt) -> dict:
    G = len(begin) - 1
    sizes = [int(begin[g + 1] - begin[g]) for g in range(G)]
    out = {}
    if lab is not None:
        out["labels"] = [lab[int(begin[g]):int(begin[g + 1])].copy() for g in range(G)]
        out["counts"] = cnt[:G].copy()
    if mats is not None:
        out["distances"], at = [], 0
        for n in sizes:
            out["distances"].append(mats[at:at + n * n].reshape(n, n).copy())
            at += n * n
    return out


def cluster_outcomes_host(robot: RobotDescription, groups, threshold: float, distances: bool = False, labels: bool = True) -> dict:
    """fks_cluster_configs: the host twin of Simulator.cluster_outcomes, with the kernels'
    arithmetic and without a context or a GPU; the same result byte for byte."""
    configs, begin = _cluster_groups(groups, robot.config_width)
    out = _cluster_outputs(begin, labels, distances)
    desc, keep = robot.to_c()
    st = _capi.lib().fks_cluster_configs(ctypes.byref(desc), _cluster_ptr(configs, ctypes.c_double), _capi.as_ptr(begin, ctypes.c_uint64),
                                         len(begin) - 1, float(threshold), _cluster_ptr(out[0], ctypes.c_double),
                                         _cluster_ptr(out[1], ctypes.c_uint32), _cluster_ptr(out[2], ctypes.c_uint32))
    del keep
    _capi.check(st, None, "fks_cluster_configs")
    return _cluster_result(begin, *out)


@dataclass
class PolicyTable:
    """fks_policy_table over host arrays: keys and targets (M, W), terminal (M,) booleans or None,
    and the two distances of the verdict (include/fks_capi.h)."""
    keys: np.ndarray
    targets: np.ndarray
    terminal: Optional[np.ndarray] = None
    terminal_distance: float = 0.0
    max_distance: float = float("inf")

    def to_c(self, W: int):
        """(fks_policy_table, the arrays its pointers refer to)."""
        keys = np.ascontiguousarray(np.asarray(self.keys, dtype=np.float64).reshape(-1, W))
        targets = np.ascontiguousarray(np.asarray(self.targets, dtype=np.float64).reshape(-1, W))
        if keys.shape != targets.shape:
            raise ValueError("a policy table's keys and targets must hold the same number of configurations")
        flags = None
        if self.terminal is not None:
            flags = np.ascontiguousarray(np.where(np.asarray(self.terminal).reshape(-1), _capi.POLICY_ENTRY_TERMINAL, 0),
                                         dtype=np.uint32)
            if flags.shape[0] != keys.shape[0]:
                raise ValueError("a policy table's terminal flags must hold one entry per key")
        table = _capi.PolicyTable(keys.ctypes.data if keys.size else None, targets.ctypes.data if targets.size else None,
                                  flags.ctypes.data if flags is not None and flags.size else None, keys.shape[0],
                                  float(self.terminal_distance), float(self.max_distance))
        return table, (keys, targets, flags)


def policy_select(robot: RobotDescription, table: PolicyTable, configs) -> dict:
    """fks_policy_select: the selection of a policy table for configs (n, W) on the host, with the
    kernels' arithmetic and without a context.  Returns "choice" uint32 [n] (an entry's index,
    alone or or-ed with POLICY_ARRIVED, or POLICY_LOST) and "distance" [n]."""
    W = robot.config_width
    q = np.ascontiguousarray(np.asarray(configs, dtype=np.float64).reshape(-1, W))
    n = q.shape[0]
    desc, keep = robot.to_c()
    ctable, keep_table = table.to_c(W)
    choice = np.zeros(n, dtype=np.uint32)
    distance = np.zeros(n, dtype=np.float64)
    st = _capi.lib().fks_policy_select(ctypes.byref(desc), ctypes.byref(ctable), _capi.as_ptr(q, ctypes.c_double), n,
                                       _capi.as_ptr(choice, ctypes.c_uint32), _capi.as_ptr(distance, ctypes.c_double))
    del keep, keep_table
    _capi.check(st, None, "fks_policy_select")
    return {"choice": choice, "distance": distance}


def _host_jobs(jobs, W: int):
    """The fks_job array of (starts, targets, allow_contacts) jobs over host arrays: the ctypes
    array, per job its (targets' count, output arrays), and the input arrays to keep alive."""
    array = (_capi.Job * max(len(jobs), 1))()
    results, keep = [], []
    for j, (start_positions, target_positions, allow_contacts) in enumerate(jobs):
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        targets = np.ascontiguousarray(np.asarray(target_positions, dtype=np.float64).reshape(-1, W))
        n = starts.shape[0]
        out = {"positions": np.zeros((n, W), dtype=np.float64), "collided": np.zeros(n, dtype=np.uint8),
               "microsteps": np.zeros(n, dtype=np.uint32), "resolver_iterations": np.zeros(n, dtype=np.uint32),
               "error_flags": np.zeros(n, dtype=np.uint32)}
        ptr = (lambda a: a.ctypes.data) if n > 0 else (lambda a: None)
        array[j] = _capi.Job(ptr(starts), n, targets.ctypes.data if targets.size else None, targets.shape[0], 0,
                             1 if allow_contacts else 0, 0, ptr(out["positions"]), ptr(out["collided"]), ptr(out["microsteps"]),
                             ptr(out["resolver_iterations"]), ptr(out["error_flags"]))
        results.append(out)
        keep.append((starts, targets))
    return array, results, keep


def _host_path_jobs(jobs, W: int):
    """The fks_path_job array of (starts, waypoints, allow_contacts) jobs over host arrays: the
    ctypes array, per job its leg-major output arrays, and the input arrays to keep alive."""
    array = (_capi.PathJob * max(len(jobs), 1))()
    results, keep = [], []
    for j, (start_positions, waypoints, allow_contacts) in enumerate(jobs):
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        n = starts.shape[0]
        way, K, nt = _path_waypoints(waypoints, W, n)
        out = {"positions": np.zeros((K, n, W), dtype=np.float64), "collided": np.zeros((K, n), dtype=np.uint8),
               "microsteps": np.zeros((K, n), dtype=np.uint32), "resolver_iterations": np.zeros((K, n), dtype=np.uint32),
               "error_flags": np.zeros((K, n), dtype=np.uint32)}
        ptr = (lambda a: a.ctypes.data) if n > 0 and K > 0 else (lambda a: None)
        array[j] = _capi.PathJob(ptr(starts), n, way.ctypes.data if way.size else None, K, nt, 0, 1 if allow_contacts else 0, 0,
                                 ptr(out["positions"]), ptr(out["collided"]), ptr(out["microsteps"]),
                                 ptr(out["resolver_iterations"]), ptr(out["error_flags"]))
        results.append(out)
        keep.append((starts, way))
    return array, results, keep


def _job_result(out: dict) -> dict:
    return {"positions": out["positions"], "collided": out["collided"].astype(bool), "microsteps": out["microsteps"],
            "resolver_iterations": out["resolver_iterations"], "error_flags": out["error_flags"]}


def _path_waypoints(waypoints, W: int, n: int):
    """The waypoints of a path as a contiguous (K, 1 or n, W) array, with K and the per-leg count."""
    way = np.asarray(waypoints, dtype=np.float64)
    if way.ndim == 2 and way.shape[0] > 0:
        way = way[:, None, :]
    if way.size == 0:
        way = way.reshape(0, 1, W)
    if way.ndim != 3 or way.shape[2] != W:
        raise ValueError("waypoints must be (legs, 1 or n, W), or (legs, W) for one shared waypoint per leg")
    if n > 0 and way.shape[1] not in (1, n):
        raise ValueError("every leg must hold 1 or len(start_positions) waypoints (SPCS:792)")
    return np.ascontiguousarray(way), int(way.shape[0]), int(way.shape[1])


class MultiDeviceSimulator:
    """One process, several MI355X devices (fks_create_multi): every batch is split into
    contiguous particle shards, one per listed device, simulated concurrently with each
    shard's first_particle_id, and gathered into one result (bit-identical to one device).
    Statistics are summed over the devices.  Replaces the reference's OpenMP particle loop
    (SPCS:795) at device granularity; one process per GPU under torch.distributed is the
    other route (sharding.py, bench.py)."""

    def __init__(self, environment: SimulatorEnvironment, solver_config: SimulatorSolverParameters,
                 simulation_controller_frequency: float, prng_seed: int, devices: Sequence[int], debug_level: int = 0):
        self._lib = _capi.lib()
        env_c, self._env_keep = environment.to_c()
        params = solver_config.to_c()
        devs = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
        ctx = ctypes.c_void_p()
        st = self._lib.fks_create_multi(ctypes.byref(env_c), ctypes.byref(params), float(simulation_controller_frequency),
                                        ctypes.c_uint64(int(prng_seed) & 0xFFFFFFFFFFFFFFFF), int(debug_level), devs, len(devices),
                                        ctypes.byref(ctx))
        _capi.check(st, None, "fks_create_multi")
        self._ctx = ctx
        self._robot = None

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.fks_destroy_multi(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st, what):
        if st != _capi.FKS_OK:
            raise _capi.FksError(st, f"{what}: {self._lib.fks_multi_get_last_error(self._ctx).decode()}")

    def num_devices(self) -> int:
        return int(self._lib.fks_multi_num_devices(self._ctx))

    def set_active_devices(self, count: int = 0):
        """Shard the batches that follow over the first `count` listed devices (0 = all;
        fks_multi_set_active_devices).  Results do not depend on it."""
        self._check(self._lib.fks_multi_set_active_devices(self._ctx, int(count)), "fks_multi_set_active_devices")

    def active_devices(self) -> int:
        return int(self._lib.fks_multi_active_devices(self._ctx))

    def device_simulator_specialization(self, shard: int = 0) -> dict:
        """fks_get_specialization of one device's context."""
        info = _capi.SpecializationInfo()
        ctx = self._lib.fks_multi_device_context(self._ctx, int(shard))
        _capi.check(self._lib.fks_get_specialization(ctx, ctypes.byref(info)), ctx, "specialization")
        return info.as_dict()

    def prepare_batched_specialization(self):
        """fks_prepare_batched_specialization on every device's context (each decides for itself)."""
        for shard in range(self.num_devices()):
            ctx = self._lib.fks_multi_device_context(self._ctx, shard)
            _capi.check(self._lib.fks_prepare_batched_specialization(ctx), ctx, "batched specialization")

    def device_simulator_batched_specialization(self, shard: int = 0) -> dict:
        """fks_get_batched_specialization of one device's context."""
        info = _capi.SpecializationInfo()
        ctx = self._lib.fks_multi_device_context(self._ctx, int(shard))
        _capi.check(self._lib.fks_get_batched_specialization(ctx, ctypes.byref(info)), ctx, "batched specialization")
        return info.as_dict()

    def set_robot(self, robot: RobotDescription):
        if self._robot is robot:
            return
        desc, keep = robot.to_c()
        self._check(self._lib.fks_multi_set_robot(self._ctx, ctypes.byref(desc)), "fks_multi_set_robot")
        self._robot = robot

    def set_call_index(self, call_index: int):
        self._check(self._lib.fks_multi_set_call_index(self._ctx, ctypes.c_uint64(int(call_index))), "call index")

    def forward_simulate_arrays(self, robot: RobotDescription, start_positions, target_positions, allow_contacts: bool) -> dict:
        self.set_robot(robot)
        W = robot.config_width
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        targets = np.ascontiguousarray(np.asarray(target_positions, dtype=np.float64).reshape(-1, W))
        n = starts.shape[0]
        out = np.zeros((n, W), dtype=np.float64)
        collided = np.zeros(n, dtype=np.uint8)
        micro = np.zeros(n, dtype=np.uint32)
        resolver = np.zeros(n, dtype=np.uint32)
        errors = np.zeros(n, dtype=np.uint32)
        st = self._lib.fks_multi_forward_simulate(
            self._ctx, _capi.as_ptr(starts, ctypes.c_double), n, _capi.as_ptr(targets, ctypes.c_double), targets.shape[0],
            1 if allow_contacts else 0, _capi.as_ptr(out, ctypes.c_double), _capi.as_ptr(collided, ctypes.c_uint8),
            _capi.as_ptr(micro, ctypes.c_uint32), _capi.as_ptr(resolver, ctypes.c_uint32), _capi.as_ptr(errors, ctypes.c_uint32))
        self._check(st, "fks_multi_forward_simulate")
        return {"positions": out, "collided": collided.astype(bool), "microsteps": micro, "resolver_iterations": resolver,
                "error_flags": errors}

    def forward_simulate_path_arrays(self, robot: RobotDescription, start_positions, waypoints, allow_contacts: bool) -> dict:
        """fks_multi_forward_simulate_path: HipParticleContactSimulator.forward_simulate_path_arrays
        sharded over the devices (bit-identical to one device)."""
        self.set_robot(robot)
        W = robot.config_width
        starts = np.ascontiguousarray(np.asarray(start_positions, dtype=np.float64).reshape(-1, W))
        n = starts.shape[0]
        way, K, nt = _path_waypoints(waypoints, W, n)
        out = np.zeros((K, n, W), dtype=np.float64)
        collided = np.zeros((K, n), dtype=np.uint8)
        micro = np.zeros((K, n), dtype=np.uint32)
        resolver = np.zeros((K, n), dtype=np.uint32)
        errors = np.zeros((K, n), dtype=np.uint32)
        st = self._lib.fks_multi_forward_simulate_path(
            self._ctx, _capi.as_ptr(starts, ctypes.c_double), n, _capi.as_ptr(way, ctypes.c_double), K, nt,
            1 if allow_contacts else 0, _capi.as_ptr(out, ctypes.c_double), _capi.as_ptr(collided, ctypes.c_uint8),
            _capi.as_ptr(micro, ctypes.c_uint32), _capi.as_ptr(resolver, ctypes.c_uint32), _capi.as_ptr(errors, ctypes.c_uint32))
        self._check(st, "fks_multi_forward_simulate_path")
        return {"positions": out, "collided": collided.astype(bool), "microsteps": micro, "resolver_iterations": resolver,
                "error_flags": errors}

    def forward_simulate_jobs_arrays(self, robot: RobotDescription, jobs) -> list:
        """fks_multi_forward_simulate_jobs: HipParticleContactSimulator.forward_simulate_jobs_arrays
        with the jobs' particles, laid end to end, sharded over the devices (bit-identical to one
        device)."""
        self.set_robot(robot)
        array, results, _keep = _host_jobs(jobs, robot.config_width)
        st = self._lib.fks_multi_forward_simulate_jobs(self._ctx, array, len(results))
        self._check(st, "fks_multi_forward_simulate_jobs")
        return [_job_result(r) for r in results]

    def forward_simulate_path_jobs_arrays(self, robot: RobotDescription, jobs) -> list:
        """fks_multi_forward_simulate_path_jobs: HipParticleContactSimulator.forward_simulate_path_jobs_arrays
        with the jobs' particles, laid end to end, sharded over the devices (bit-identical to one
        device)."""
        self.set_robot(robot)
        array, results, _keep = _host_path_jobs(jobs, robot.config_width)
        st = self._lib.fks_multi_forward_simulate_path_jobs(self._ctx, array, len(results))
        self._check(st, "fks_multi_forward_simulate_path_jobs")
        return [_job_result(r) for r in results]

    def check_config_collisions(self, robot: RobotDescription, configs, inflation_ratio: float):
        """Batched CheckConfigCollision (SPCS:1398-1416) sharded over the devices:
        (collided bool[n], error bits uint32[n])."""
        self.set_robot(robot)
        W = robot.config_width
        c = np.ascontiguousarray(np.asarray(configs, dtype=np.float64).reshape(-1, W))
        n = c.shape[0]
        collided = np.zeros(n, dtype=np.uint8)
        errors = np.zeros(n, dtype=np.uint32)
        st = self._lib.fks_multi_check_config_collision(self._ctx, _capi.as_ptr(c, ctypes.c_double), n, float(inflation_ratio),
                                                        _capi.as_ptr(collided, ctypes.c_uint8), _capi.as_ptr(errors, ctypes.c_uint32))
        self._check(st, "fks_multi_check_config_collision")
        return collided.astype(bool), errors

    def get_statistics(self) -> dict:
        s = _capi.Statistics()
        self._check(self._lib.fks_multi_get_statistics(self._ctx, ctypes.byref(s)), "statistics")
        return s.as_dict()

    def last_call_counters(self) -> dict:
        c = _capi.CallCounters()
        self._check(self._lib.fks_multi_get_last_call_counters(self._ctx, ctypes.byref(c)), "counters")
        return c.as_dict()


def _marker(ns, marker_id, marker_type, frame, scale, color):
    """A visualization_msgs::Marker as a plain dict (ROS is not part of this repository)."""
    return {"ns": ns, "id": int(marker_id), "type": marker_type, "action": "ADD", "frame_id": frame,
            "frame_locked": False, "scale": [float(v) for v in scale], "color": list(color),
            "pose": {"position": [0.0, 0.0, 0.0], "orientation": [0.0, 0.0, 0.0, 1.0]}, "points": None, "colors": None}


def _make(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level, device=0):
    return HipParticleContactSimulator(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level, device)


def make_se2_simulator(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level=0, device=0):
    """fast_kinematic_simulator::MakeSE2Simulator (FKS.cpp:4-25)."""
    return _make(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level, device)


def make_se3_simulator(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level=0, device=0):
    """fast_kinematic_simulator::MakeSE3Simulator (FKS.cpp:27-48)."""
    return _make(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level, device)


def make_linked_simulator(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level=0, device=0):
    """fast_kinematic_simulator::MakeLinkedSimulator (FKS.cpp:50-71)."""
    return _make(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level, device)
