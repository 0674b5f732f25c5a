/*
 * fks_capi.h — C-ABI of the MI355X-native particle forward-simulation path.
 *
 * This is the drop-in boundary that replaces the OpenMP particle loop of
 * simple_particle_contact_simulator::SimpleParticleContactSimulator
 * (reference: include/fast_kinematic_simulator/simple_particle_contact_simulator.hpp,
 * abbreviated SPCS below).  Plain C types only: no C++, no torch, no HIP types
 * cross this header.  A C++ host wrapper that re-implements the
 * uncertainty_planning_core SimulatorInterface on top of these entry points is in
 * include/fast_kinematic_simulator_amd/hip_particle_contact_simulator.hpp and the
 * Python mirror is fast_kinematic_simulator_amd/simulator.py.
 *
 * Entry point  ->  reference interface it replaces
 *   fks_default_solver_params  -> fast_kinematic_simulator::GetDefaultSolverParameters   (FKS.hpp:13-16)
 *   fks_create + fks_set_robot -> fast_kinematic_simulator::Make{SE2,SE3,Linked}Simulator (FKS.cpp:4-71),
 *                                 SimpleParticleContactSimulator ctor (SPCS:420-444)
 *   fks_forward_simulate       -> SimpleParticleContactSimulator::ForwardSimulateRobots (SPCS:788-804)
 *   fks_reverse_simulate       -> SimpleParticleContactSimulator::ReverseSimulateRobots (SPCS:806-822)
 *   fks_forward_simulate_device-> same as fks_forward_simulate, inputs/outputs already in HBM
 *   fks_forward_simulate_path  -> the planner's loop of ForwardSimulateRobots calls over a waypoint list
 *                                 (no single reference function), in one launch
 *   fks_forward_simulate_jobs  -> the planner's independent ForwardSimulateRobots / ReverseSimulateRobots
 *                                 calls (tree extensions, edge attempts, policy roll-outs), in one launch
 *   fks_check_config_collision -> SimpleParticleContactSimulator::CheckConfigCollision   (SPCS:1398-1416),
 *                                 batched (one call per configuration in the reference)
 *   fks_get_statistics         -> SimpleParticleContactSimulator::GetStatistics          (SPCS:488-500)
 *   fks_reset_statistics       -> SimpleParticleContactSimulator::ResetStatistics        (SPCS:502-512)
 *   fks_reset_generators       -> SimpleParticleContactSimulator::ResetGenerators        (SPCS:457-471)
 *   fks_get/set_debug_level    -> Get/SetDebugLevel                                       (SPCS:446-455)
 *   fks_env_build              -> simulator_environment_builder::BuildCompleteEnvironment
 *                                 (src/.../simulator_environment_builder.cpp:470-476; CPU preprocessing)
 *
 * Errors: every call returns fks_status; fks_get_last_error() gives the text.
 * Nothing throws across the ABI.  Per-particle problems that the reference
 * handles with assert() (SPCS:1570-1575, 1882, GetBestSurfaceNormal SPCS:113-114)
 * are reported as FKS_PARTICLE_ERR_* bits and that particle stops simulating.
 *
 * Threading: a context is single-caller and stream-ordered (the reference's
 * simulator object is not safe for concurrent calls either, SPCS:846-850).
 */
#ifndef FKS_CAPI_H
#define FKS_CAPI_H

#if defined(__HIPCC_RTC__)
/* run-time compilation of shape-specialised kernels (fks_specialize): hiprtc's prelude
 * declares the fixed-width types in its own namespace and has no libc headers */
using __hip_internal::int16_t;
using __hip_internal::int32_t;
using __hip_internal::int64_t;
using __hip_internal::int8_t;
using __hip_internal::uint16_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
using __hip_internal::uint8_t;
#ifndef INT32_MIN
#define INT32_MIN (-2147483647 - 1)
#endif
#else
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* 5: the opt-in joint-space proof (ABI 4: fks_set_joint_proof, fks_call_counters.
 * proven_free_microsteps) removed: it broke even on the headline.
 * 6: host robot control (fks_robot_control_action, fks_robot_apply_control_input), the
 * environment builder's public steps (fks_env_discretize_obstacle, fks_env_build_normals,
 * fks_env_cell_objects), fks_set_statistics / fks_set_total_counters.
 * 7: fks_set_small_batch_kernel
 * 8: shape specialisation, launch info
 * 9: specialisation modes (FKS_SPECIALIZE_NO_PROOFS validation kernel), build failures in
 *    fks_specialization_info (failed, message), fks_multi_set_active_devices, pinned per-device
 *    staging in fks_multi_*
 * 10: cooperative small batches (fks_set_cooperative_waves, FKS_KERNEL_COOPERATIVE, launch
 *    info cooperative_*), the shape-specialised small-batch kernel (FKS_KERNEL_SHAPED_SMALL_BATCH),
 *    fks_set_segment_heavy_relative */
#define FKS_ABI_VERSION 10

typedef enum {
    FKS_OK = 0,
    FKS_ERR_INVALID_ARGUMENT = 1,
    FKS_ERR_HIP = 2,
    FKS_ERR_NO_ROBOT = 3,
    FKS_ERR_OUT_OF_MEMORY = 4,
    FKS_ERR_UNSUPPORTED = 5,
    FKS_ERR_NO_DEVICE = 6
} fks_status;

typedef enum { FKS_ROBOT_LINKED = 0, FKS_ROBOT_SE2 = 1, FKS_ROBOT_SE3 = 2 } fks_robot_type;

/* arc_utilities simple_linked_robot_model::SimpleJointModel::JOINT_TYPE values */
typedef enum {
    FKS_JOINT_FIXED = 0,
    FKS_JOINT_REVOLUTE = 1,
    FKS_JOINT_CONTINUOUS = 2,
    FKS_JOINT_PRISMATIC = 4
} fks_joint_type;

/* per-particle error bits (replace the reference's asserts) */
#define FKS_PARTICLE_ERR_MICROSTEP_MOTION 0x1u   /* SPCS:1570-1575 computed microstep motion > allowed  */
#define FKS_PARTICLE_ERR_NORMAL_OOB 0x2u         /* SPCS:1882 surface normal lookup out of bounds        */
#define FKS_PARTICLE_ERR_ZERO_DIRECTION 0x4u     /* SPCS:113-114 best-normal query with zero motion      */
#define FKS_PARTICLE_ERR_RNG_EXHAUSTED 0x8u      /* truncated-normal rejection exceeded its draw budget  */
#define FKS_PARTICLE_ERR_SELF_CAPACITY 0x10u     /* reserved: ABI <= 2 capped the self-collision impulse
                                                    solve; since ABI 3 it is unbounded (never raised)    */
#define FKS_PARTICLE_ERR_KEY_RANGE 0x20u         /* non-finite point in the self-collision grid          */
#define FKS_PARTICLE_ERR_MICROSTEP_CAP 0x40u     /* microsteps per controller step exceeded 2^20         */
#define FKS_PARTICLE_ERR_SELF_SINGULAR 0x80u     /* NaN self-collision correction (assert SPCS:1151-1153) */
#define FKS_PARTICLE_ERR_NO_NOISE_BIN 0x100u     /* sampled actuator: no bin holds the command (UNC:152-153) */

/* SimulatorSolverParameters (SPCS:345-369); booleans widened to uint32 */
typedef struct {
    double forward_simulation_time;
    double simulation_shortcut_distance;
    double environment_collision_check_tolerance;
    double resolve_correction_step_scaling_decay_rate;
    double resolve_correction_initial_step_size;
    double resolve_correction_min_step_scaling;
    uint32_t max_resolver_iterations;
    uint32_t resolve_correction_step_scaling_decay_iterations;
    uint32_t failed_resolves_end_motion;
    uint32_t reserved;
} fks_solver_params;

/* A VoxelGrid geometry (arc_utilities VoxelGrid): origin transform as a 3x4
 * row-major [R | t], cubic cells, cell counts; storage index
 * (x * ny + y) * nz + z (z fastest). */
typedef struct {
    double origin[12];
    double resolution;
    int64_t num_cells[3];
} fks_grid_geometry;

/* The three inputs the reference simulator copies at construction (SPCS:379-381):
 * environment_ (collision map: only its geometry is used on the path: GetResolution
 * SPCS:524-527 and GetInverseOriginTransform SPCS:1176), environment_sdf_
 * (float distance per cell, oob_value returned outside, SEB.cpp:473 uses +inf) and
 * surface_normals_grid_ (SPCS:44-343, stored as CSR: cell c owns entries
 * [normal_offsets[c], normal_offsets[c+1]); each entry is 6 doubles: the
 * SafeNormal'ed entry direction xyz (its w is always 0) then the SafeNormal'ed
 * normal xyz, in insertion order).  Arrays are read during fks_create/fks_env
 * upload only; the caller keeps ownership. */
typedef struct {
    fks_grid_geometry collision_map;
    fks_grid_geometry sdf;
    const float* sdf_values;
    float sdf_oob_value;
    uint32_t reserved;
    fks_grid_geometry normals;
    const uint32_t* normal_offsets; /* num_cells+1 entries */
    const double* normal_entries;   /* 6 * normal_offsets[num_cells] doubles */
} fks_environment;

/* TnuvaLinkedRobot::LINKED_ROBOT_CONFIG (TNUVA:420-457); SE2/SE3 use one per axis */
typedef struct {
    double kp;
    double ki;
    double kd;
    double integral_clamp;
    double velocity_limit;
    double acceleration_limit;
    double max_sensor_noise;
    double max_actuator_proportional_noise;
    double max_actuator_minimum_noise;
} fks_dof_controller;

/* SampledUncertainVelocityActuator (UNC:123-281): bins of observed velocity errors
 * keyed by commanded velocity (JointUncertaintySampleModel, UNC:123).  Bin k covers
 * [bin_bounds[2k], bin_bounds[2k+1]]; the first bin holding the clamped command
 * wins (GetMatchingBin, UNC:140-154) and one of its bin_elements samples, picked
 * uniformly, is added to it (GetNoiseValue, UNC:228-243).  num_bins == 0 keeps the
 * truncated-normal actuator of fks_dof_controller for that dof. */
typedef struct {
    uint32_t num_bins;
    uint32_t bin_elements;
    const double* bin_bounds;  /* num_bins x (lower, upper) */
    const double* bin_samples; /* num_bins x bin_elements */
} fks_sampled_actuator;

/* simple_linked_robot_model::RobotJoint */
typedef struct {
    int32_t parent_link;
    int32_t child_link;
    int32_t type; /* fks_joint_type */
    int32_t reserved;
    double origin[12]; /* parent link frame -> joint frame, 3x4 row-major */
    double axis[3];
    double limit_lower;
    double limit_upper;
} fks_joint_desc;

/* Flattened robot.  Geometries are the robot_link_geometries vector
 * (GetLinkGeometries): geometry g belongs to link geometry_link[g] and owns
 * points [geometry_point_offset[g], geometry_point_offset[g+1]) of `points`
 * (x, y, z, w per point: PointSphereGeometry POINTS with w = 1).  Allowed
 * self-collision pairs are given as geometry indices (the indices that
 * CheckIfSelfCollisionAllowed receives at SPCS:1008,1193).
 *  linked: num_dofs = number of non-fixed joints, configuration = joint values
 *  SE2:    num_dofs = 3, configuration = (x, y, theta), controllers = x, y, theta
 *  SE3:    num_dofs = 6, configuration = 3x4 row-major pose (12 doubles),
 *          controllers = x, y, z, rx, ry, rz (twist order, TNUVA:352-358)
 * distance_weights: linked -> one weight per dof; SE2/SE3 -> [position, rotation]. */
typedef struct {
    int32_t robot_type; /* fks_robot_type */
    int32_t num_links;
    int32_t num_joints;
    int32_t num_geometries;
    int32_t num_dofs;
    int32_t num_allowed_pairs;
    double base_transform[12];
    const fks_joint_desc* joints;
    const int32_t* geometry_link;
    const uint32_t* geometry_point_offset;
    const double* points;
    const int32_t* allowed_pairs;
    const fks_dof_controller* controllers;
    const double* distance_weights;
    /* NULL, or num_dofs entries: per-dof SampledUncertainVelocityActuator (ABI 2) */
    const fks_sampled_actuator* sampled_actuators;
} fks_robot_desc;

/* SimpleParticleContactSimulator statistics counters (SPCS:392-400, 488-500) */
typedef struct {
    uint64_t successful_resolves;
    uint64_t unsuccessful_resolves;
    uint64_t free_resolves;
    uint64_t collision_resolves;
    uint64_t fallback_resolves;
    uint64_t unsuccessful_env_collision_resolves;
    uint64_t unsuccessful_self_collision_resolves;
    uint64_t recovered_unsuccessful_resolves;
} fks_statistics;

/* Work/traffic counters of the last forward/reverse call (all particles). */
typedef struct {
    uint64_t particles;
    uint64_t controller_steps;
    uint64_t microsteps;          /* executions of the microstep loop body, SPCS:1590-1796 */
    uint64_t resolver_iterations; /* executions of the resolver loop body, SPCS:1625-1762 */
    uint64_t sdf_bytes;           /* algorithmic SDF/normal-grid bytes the reference would read */
    uint64_t error_particles;
    double kernel_ms;             /* device time of the simulation kernel (HIP events) */
    double call_ms;               /* host wall time of the whole call */
    uint64_t calls;               /* number of calls these counters cover */
    uint64_t least_squares_rows;  /* sum over resolver iterations of the stacked-Jacobian rows (3 x corrected points) */
    /* ABI 3: the self-collision branch of the resolver (SPCS:983-1275) */
    uint64_t self_collision_checks; /* CheckCollision calls (SPCS:1418-1436) whose self-collision map came back
                                       non-empty, i.e. ExtractSelfCollidingPoints produced corrections (SPCS:1264-1271) */
    uint64_t self_corrected_points; /* sum over resolver iterations of the points whose correction holds a
                                       self-collision term (SPCS:1846-1853, 1909-1916) */
    uint64_t reserved0;             /* ABI 4's proven_free_microsteps (removed in ABI 5); always 0 */
} fks_call_counters;

typedef struct fks_context fks_context;

int fks_abi_version(void);
const char* fks_status_string(fks_status status);

/* GetDefaultSolverParameters (FKS.hpp:13-16) */
fks_status fks_default_solver_params(fks_solver_params* out);

/* Make{SE2,SE3,Linked}Simulator (FKS.cpp:4-71): copies env to device `device`.
 * The stacked-Jacobian resolver is always used (FKS.cpp:22,45,68 pass false). */
fks_status fks_create(const fks_environment* env, const fks_solver_params* params,
                      double simulation_controller_frequency, uint64_t prng_seed,
                      int32_t debug_level, int32_t device, fks_context** out_ctx);
void fks_destroy(fks_context* ctx);
const char* fks_get_last_error(const fks_context* ctx);

/* Upload/replace the robot every particle is a clone of (the immutable_robot
 * argument of ForwardSimulateRobots, SPCS:788).  Cached until replaced. */
fks_status fks_set_robot(fks_context* ctx, const fks_robot_desc* robot);
/* configuration width in doubles for the current robot (linked D, SE2 3, SE3 12) */
int32_t fks_config_width(const fks_context* ctx);

/* ForwardSimulateRobots (SPCS:788): host buffers.  starts: n*W doubles;
 * targets: num_targets*W doubles with num_targets == 1 or n (SPCS:792).
 * Outputs (n entries each, any may be NULL except out_positions):
 * reached configuration, collided flag (SimulationResult), microsteps,
 * resolver iterations and FKS_PARTICLE_ERR_* bits per particle. */
fks_status fks_forward_simulate(fks_context* ctx, const double* starts, uint64_t n,
                                const double* targets, uint64_t num_targets,
                                int32_t allow_contacts, double* out_positions,
                                uint8_t* out_collided, uint32_t* out_microsteps,
                                uint32_t* out_resolver_iterations, uint32_t* out_error_flags);
/* ReverseSimulateRobots (SPCS:806): identical semantics (SPCS:838-841). */
fks_status fks_reverse_simulate(fks_context* ctx, const double* starts, uint64_t n,
                                const double* targets, uint64_t num_targets,
                                int32_t allow_contacts, double* out_positions,
                                uint8_t* out_collided, uint32_t* out_microsteps,
                                uint32_t* out_resolver_iterations, uint32_t* out_error_flags);

/* ForwardSimulateMutableRobot (SPCS:843-919) / ReverseSimulateMutableRobot (SPCS:838-841)
 * for a batch: particle i starts from starts[i] (SetPosition: joint limits / angle wrap)
 * with its PID controllers as the robot holds them, not zeroed as ResetPosition does
 * (TNUVA:524-536).  controller_state (n x 2D doubles, in/out): per dof the controller's
 * error integral, then per dof its last error (SimplePIDController PID:53-136; D = dofs, 3 for
 * SE(2), 6 for SE(3)); on return it holds each particle's controllers when it stopped.
 * All zeros gives fks_forward_simulate's results. */
fks_status fks_forward_simulate_mutable(fks_context* ctx, const double* starts, uint64_t n, const double* targets,
                                        uint64_t num_targets, int32_t allow_contacts, double* controller_state,
                                        double* out_positions, uint8_t* out_collided, uint32_t* out_microsteps,
                                        uint32_t* out_resolver_iterations, uint32_t* out_error_flags);

/* Same call with every buffer already in device memory of the context's GPU.
 * first_particle_id: global id of particle 0 of this shard (the RNG stream is
 * keyed by global id, so sharding across GPUs does not change results).
 * stream: a hipStream_t (NULL = default stream); the call returns once the
 * work is enqueued unless `synchronize` is non-zero. */
fks_status fks_forward_simulate_device(fks_context* ctx, const double* d_starts, uint64_t n,
                                       const double* d_targets, uint64_t num_targets,
                                       uint64_t first_particle_id, int32_t allow_contacts,
                                       double* d_out_positions, uint8_t* d_out_collided,
                                       uint32_t* d_out_microsteps,
                                       uint32_t* d_out_resolver_iterations,
                                       uint32_t* d_out_error_flags, void* stream,
                                       int32_t synchronize);

/* A batch along a waypoint path in one launch (added within ABI 10).  With the context at call
 * index c, the call returns byte for byte what this chain of plain calls returns, and
 * leaves the call index at c + num_legs:
 *     q_0 = starts
 *     leg k = 0 .. num_legs-1:  fks_set_call_index(c + k);
 *                               r_k = fks_forward_simulate(q_k, waypoints[k], allow_contacts);
 *                               q_{k+1} = r_k positions
 * so every leg begins with ResetPosition(q_k) (controllers zeroed, joint limits / angle wrap
 * applied again), its collided flag, counts and error bits are its own, and a leg that ends
 * early (failed resolve, contact with allow_contacts == 0, shortcut distance, error bit)
 * hands the configuration it returned to the next leg.  A particle starts leg k+1 when its
 * own leg k ends: no leg waits for the batch.
 * waypoints: [num_legs][num_targets][W] doubles, num_targets == 1 or n for every leg.
 * Outputs are leg-major: out_positions [num_legs][n][W] (required: leg k's slice is leg
 * k+1's start), the other four [num_legs][n] (each may be NULL).
 * fks_get_statistics and the work counters of fks_get_last_call_counters grow by the chain's
 * sums; `calls` counts 1.  num_legs == 0, or more legs than the segment counter holds
 * (num_legs x segments per leg < 2^31), is FKS_ERR_INVALID_ARGUMENT; n == 0 succeeds and
 * consumes num_legs call indices.  A context with fks_set_individual_jacobians on returns
 * FKS_ERR_UNSUPPORTED.  fks_set_segment_steps / _policy / _heavy_relative and
 * fks_set_small_batch_kernel apply as to a plain call (fks_set_cooperative_waves does not);
 * the call runs the robot's batched shape-specialised module when that serves it
 * (fks_prepare_batched_specialization: FKS_KERNEL_SHAPED_PATH_JOBS[_SMALL_BATCH]) and the
 * generic path kernels (FKS_KERNEL_PATH / FKS_KERNEL_PATH_SMALL_BATCH) otherwise. */
fks_status fks_forward_simulate_path(fks_context* ctx, const double* starts, uint64_t n, const double* waypoints,
                                     uint64_t num_legs, uint64_t num_targets, int32_t allow_contacts,
                                     double* out_positions, uint8_t* out_collided, uint32_t* out_microsteps,
                                     uint32_t* out_resolver_iterations, uint32_t* out_error_flags);
/* Same with device buffers (see fks_forward_simulate_device): rows [a, b) of a path with
 * first_particle_id = a equal the same rows of the whole path. */
fks_status fks_forward_simulate_path_device(fks_context* ctx, const double* d_starts, uint64_t n, const double* d_waypoints,
                                            uint64_t num_legs, uint64_t num_targets, uint64_t first_particle_id,
                                            int32_t allow_contacts, double* d_out_positions, uint8_t* d_out_collided,
                                            uint32_t* d_out_microsteps, uint32_t* d_out_resolver_iterations,
                                            uint32_t* d_out_error_flags, void* stream, int32_t synchronize);

/* Many independent calls in one launch (added within ABI 10).  A job is one plain call's
 * arguments: its start configurations (n may be 0), its targets (num_targets == 1 or n), its
 * allow_contacts and its own five output arrays.  first_particle_id is 0 for a whole job; a
 * shard of a job passes its range's start, as fks_forward_simulate_device does. */
typedef struct {
    const double* starts;
    uint64_t n;
    const double* targets;
    uint64_t num_targets; /* 1 or n */
    uint64_t first_particle_id;
    int32_t allow_contacts;
    int32_t reserved;
    double* out_positions; /* [n][W], required when n > 0 */
    uint8_t* out_collided; /* the other four [n], each may be NULL */
    uint32_t* out_microsteps;
    uint32_t* out_resolver_iterations;
    uint32_t* out_error_flags;
} fks_job;
#define FKS_MAX_JOBS 65536u
/* With the context at call index c, a batch of num_jobs jobs returns byte for byte what this
 * sequence of plain calls returns, and leaves the call index at c + num_jobs:
 *     j = 0 .. num_jobs-1:  fks_set_call_index(c + j);
 *                           r_j = fks_forward_simulate(starts_j, n_j, targets_j, num_targets_j, allow_contacts_j, ...)
 * so job j draws its noise under the key of call c + j with particle ids first_particle_id_j +
 * local, and a job's particles never interact with another job's.  The jobs' particles share
 * the device side by side: the batch lasts about as long as one plain call over all of them.
 * An empty job launches nothing and consumes its call index; when every job is empty the call
 * succeeds, launches nothing and consumes num_jobs call indices.  ReverseSimulateRobots has
 * the semantics of ForwardSimulateRobots (SPCS:838-841), so there is no reverse entry.
 * fks_get_statistics and the work counters of fks_get_last_call_counters grow by the
 * sequence's sums; `calls` counts 1 and `particles` the sum of n.
 * Refused before anything is staged or counted, with the call index unchanged and the reason in
 * fks_get_last_error: num_jobs == 0, num_jobs > FKS_MAX_JOBS (65,536), a job whose num_targets
 * is neither 1 nor n, a job with n > 0 and a NULL starts, targets or out_positions, or a sum of
 * n above 2^32-1 (FKS_ERR_INVALID_ARGUMENT); no robot set (FKS_ERR_NO_ROBOT); a context with
 * fks_set_individual_jacobians on (FKS_ERR_UNSUPPORTED).
 * Every job has a kernel-argument record (sizeof(SimArgs), 1,824 bytes) in pinned host memory and
 * in HBM, kept by the context once grown: the 65,536 cap bounds them at about 114 MiB each.
 * The kernel is chosen as a plain call over the sum of n would choose it: the small-batch jobs
 * kernel (FKS_KERNEL_JOBS_SMALL_BATCH) when the sum fits small_batch_resident_waves, no
 * segments are set, the block is not lean and fks_set_small_batch_kernel is on; the throughput
 * jobs kernel (FKS_KERNEL_JOBS) otherwise.  fks_set_segment_steps / _policy / _heavy_relative
 * apply as to a plain call over the sum; fks_set_cooperative_waves does not apply.  With the
 * robot's batched shape-specialised module (fks_prepare_batched_specialization) the same choice
 * runs its kernels instead (FKS_KERNEL_SHAPED_PATH_JOBS[_SMALL_BATCH]).
 * Host buffers: every job's inputs go up in one copy and each output array comes down in one. */
fks_status fks_forward_simulate_jobs(fks_context* ctx, const fks_job* jobs, uint64_t num_jobs);
/* Same with the job array on the host and every pointer in it in HBM (see
 * fks_forward_simulate_device for stream and synchronize): rows [a, b) of a job passed with
 * first_particle_id = a equal the same rows of the whole job. */
fks_status fks_forward_simulate_jobs_device(fks_context* ctx, const fks_job* jobs, uint64_t num_jobs, void* stream,
                                            int32_t synchronize);

/* Many independent waypoint paths in one launch (added within ABI 10).  A path job is one
 * fks_forward_simulate_path call's arguments: its start configurations (n may be 0), its
 * waypoints, its own number of legs (jobs may differ in length), its allow_contacts and its own
 * five leg-major output arrays.  first_particle_id is 0 for a whole job; a shard of a job passes
 * its range's start, and the shard's own n is its leg stride. */
typedef struct {
    const double* starts;       /* [n][W] */
    uint64_t n;                 /* may be 0 */
    const double* waypoints;    /* [num_legs][num_targets][W] */
    uint64_t num_legs;          /* >= 1 */
    uint64_t num_targets;       /* 1 or n, for every leg */
    uint64_t first_particle_id; /* 0 for a whole job; a shard passes its range's start */
    int32_t allow_contacts;
    int32_t reserved;
    double* out_positions; /* [num_legs][n][W], required when n > 0 */
    uint8_t* out_collided; /* the other four [num_legs][n], each may be NULL */
    uint32_t* out_microsteps;
    uint32_t* out_resolver_iterations;
    uint32_t* out_error_flags;
} fks_path_job;
/* the sum of num_legs over a batch: one kernel-argument record per (job, leg), so the records'
 * pinned and HBM staging keeps the bound of FKS_MAX_JOBS (about 114 MiB each) */
#define FKS_MAX_PATH_JOB_LEGS FKS_MAX_JOBS
/* With the context at call index c and K_j = jobs[j].num_legs, a batch returns byte for byte what
 * this sequence of path calls returns, and leaves the call index at c + K_0 + ... + K_{J-1}:
 *     j = 0 .. num_jobs-1:  fks_set_call_index(c + K_0 + ... + K_{j-1});
 *                           fks_forward_simulate_path(starts_j, n_j, waypoints_j, K_j, num_targets_j, allow_contacts_j, ...)
 * so leg k of job j draws its noise under the key of call c + K_0 + ... + K_{j-1} + k with
 * particle ids first_particle_id_j + local, and every leg begins with ResetPosition of what the
 * leg before returned (fks_forward_simulate_path).  With every K_j == 1 the call returns what
 * fks_forward_simulate_jobs returns, with one job what fks_forward_simulate_path returns.
 * An empty job launches nothing and consumes its K_j call indices; when every job is empty the
 * call succeeds, launches nothing and consumes them all.  fks_get_statistics and the work
 * counters of fks_get_last_call_counters grow by the sequence's sums; `calls` counts 1 and
 * `particles` the sum of n_j x K_j.
 * Refused before anything is staged or counted, with the call index unchanged and the reason in
 * fks_get_last_error: num_jobs == 0, num_jobs > FKS_MAX_JOBS, a job with num_legs == 0, a sum of
 * num_legs above FKS_MAX_PATH_JOB_LEGS, a job whose num_targets is neither 1 nor n, a job with
 * n > 0 and a NULL starts, waypoints or out_positions, a sum of n above 2^32-1, or the longest
 * job's legs x segments per leg >= 2^31 (FKS_ERR_INVALID_ARGUMENT); no robot set
 * (FKS_ERR_NO_ROBOT); a context with fks_set_individual_jacobians on (FKS_ERR_UNSUPPORTED).
 * The kernel is chosen as a plain call over the sum of n would choose it: the small-batch kernel
 * (FKS_KERNEL_PATH_JOBS_SMALL_BATCH) when the sum fits small_batch_resident_waves, no segments
 * are set, the block is not lean and fks_set_small_batch_kernel is on; the throughput kernel
 * (FKS_KERNEL_PATH_JOBS) otherwise.  fks_set_segment_steps / _policy / _heavy_relative apply as
 * to a plain call over the sum; fks_set_cooperative_waves does not apply.  With the robot's
 * batched shape-specialised module (fks_prepare_batched_specialization) the same choice runs
 * its kernels instead (FKS_KERNEL_SHAPED_PATH_JOBS[_SMALL_BATCH]).
 * Host buffers: every job's starts and waypoints go up in one copy and each output array comes
 * down in one. */
fks_status fks_forward_simulate_path_jobs(fks_context* ctx, const fks_path_job* jobs, uint64_t num_jobs);
/* Same with the job array on the host and every pointer in it in HBM (see
 * fks_forward_simulate_device for stream and synchronize): rows [a, b) of a job passed with
 * first_particle_id = a equal the same rows of the whole job. */
fks_status fks_forward_simulate_path_jobs_device(fks_context* ctx, const fks_path_job* jobs, uint64_t num_jobs, void* stream,
                                                 int32_t synchronize);

/* A policy table (added within ABI 10): the planner's execution policy as the roll-out reads it
 * (SimulateExectionPolicy / QueryBestAction): M policy states, each with the configuration it
 * stands for (its key) and its action, the configuration to move to next (its target).
 * Selection of a configuration q:
 *     p   = the position ResetPosition(q) leaves (joint limits clamped, continuous dofs and the
 *           SE(2) angle wrapped), as every simulation call does to its starts
 *     d_i = the robot's configuration distance from p to keys[i] (ComputeConfigurationDistanceTo,
 *           the simulation shortcut's own arithmetic, SPCS:898, with the robot's distance_weights)
 *     the choice is the i of the smallest d_i, compared with a strict < from +inf in ascending
 *     i: the lowest index wins a tie, and a NaN distance never wins
 *     no d_i < +inf, or d > max_distance            -> FKS_POLICY_LOST (tested first)
 *     entry TERMINAL and d < terminal_distance      -> i | FKS_POLICY_ARRIVED (strict, as SPCS:899)
 *     otherwise                                     -> i */
#define FKS_POLICY_ENTRY_TERMINAL 0x1u
typedef struct {
    const double* keys;       /* [M][W]: the policy states' configurations */
    const double* targets;    /* [M][W]: the action of each state: the next target */
    const uint32_t* flags;    /* [M] FKS_POLICY_ENTRY_* bits, or NULL (= all 0) */
    uint64_t num_entries;     /* M, 1 .. 2^30 */
    double terminal_distance; /* arrived: the nearest entry is TERMINAL and d < this */
    double max_distance;      /* lost: d > this (+inf: never) */
} fks_policy_table;
#define FKS_POLICY_ARRIVED 0x80000000u /* or-ed onto the entry's index */
#define FKS_POLICY_LOST 0xFFFFFFFEu
#define FKS_POLICY_NONE 0xFFFFFFFFu /* no selection: the particle had stopped */
#define FKS_MAX_POLICY_ENTRIES (1ull << 30)
/* The selection above for n configurations (configs [n][W]) on the host, without a context (as
 * fks_robot_control_action): out_choice [n] (required) receives the verdicts, out_distance [n]
 * (may be NULL) the chosen entry's d (+inf for a table without a finite distance).  The same
 * expression trees as the policy kernels (shared SE(3) primitives and portable libm), so it is
 * the planner's single query during real execution (QueryBestAction) and the host twin the
 * roll-out's choices and distances equal bit for bit.  FKS_ERR_INVALID_ARGUMENT for a malformed
 * robot or table (NULL keys or targets, M == 0 or above 2^30, a NaN distance) or a NULL configs
 * or out_choice with n > 0. */
fks_status fks_policy_select(const fks_robot_desc* robot, const fks_policy_table* table, const double* configs, uint64_t n,
                             uint32_t* out_choice, double* out_distance);
/* A batch rolled out under a policy table in one launch (added within ABI 10): closed loop, so
 * two particles of one batch may take different routes.  With the context at call index c and
 * K = max_legs, the call returns byte for byte what this sequence returns, and leaves the call
 * index at c + K:
 *     q_0 = starts; every particle active
 *     leg k = 0 .. K-1:
 *         every active particle p: choice[k][p], distance[k][p] = selection of q_k[p];
 *             FKS_POLICY_LOST or ..._ARRIVED: p stops, legs_run[p] = k
 *         the still-active particles, each under its own particle id, at call index c + k:
 *             fks_forward_simulate(q_k[p] -> table.targets[choice[k][p]], allow_contacts)
 *         q_{k+1}[p] = that call's position
 *     particles that ran all K legs: legs_run[p] = K; choice[K][p], distance[K][p] = selection of q_K[p]
 * Every leg begins with ResetPosition (controllers zeroed), and a leg that ends early (shortcut
 * distance, failed resolve, contact with allow_contacts == 0, error bit) hands its configuration
 * to the next selection, as a path's does.  A particle starts its next leg when its own leg
 * ends: no leg waits for the batch.
 * Outputs: the five simulation outputs are leg-major as a path's, out_positions [K][n][W]
 * (required), the other four [K][n] (each may be NULL); out_choice uint32 [K+1][n] (required),
 * out_distance double [K+1][n] and out_legs_run uint32 [n] (each may be NULL).  Rows a particle
 * does not run (legs >= legs_run[p]) are defined: its position rows hold the bytes of the
 * configuration handed over at the stop (q_{legs_run}[p], unchanged), so the last leg's slice
 * always holds where the particle is; collided, microsteps, resolver iterations and error flags
 * are 0; out_choice rows after row legs_run[p] are FKS_POLICY_NONE and their distance +inf.
 * fks_get_statistics and the work counters of fks_get_last_call_counters grow by the sums of the
 * simulated (particle, leg) pairs; `calls` counts 1 and `particles` those pairs.  n == 0 succeeds
 * and consumes K call indices.
 * Refused before anything is staged or counted, with the call index unchanged and the reason in
 * fks_get_last_error: max_legs == 0, max_legs x segments per leg >= 2^31, M == 0 or M > 2^30,
 * NULL keys or targets, a NULL out_choice or out_positions (or starts) with n > 0, a NaN
 * terminal_distance or max_distance (FKS_ERR_INVALID_ARGUMENT); no robot set (FKS_ERR_NO_ROBOT); a
 * context with fks_set_individual_jacobians on (FKS_ERR_UNSUPPORTED).
 * The kernel is chosen as a path's over n: the small-batch policy kernel
 * (FKS_KERNEL_POLICY_SMALL_BATCH) when n fits small_batch_resident_waves, no segments are set,
 * the block is not lean and fks_set_small_batch_kernel is on; the throughput one
 * (FKS_KERNEL_POLICY) otherwise.  fks_set_segment_steps / _policy / _heavy_relative apply as to a
 * path; the call always runs these generic kernels, also when a batched shaped module exists.
 * Host buffers: the table goes up with the starts in one copy and each output array comes down
 * in one. */
fks_status fks_forward_simulate_policy(fks_context* ctx, const double* starts, uint64_t n, const fks_policy_table* table,
                                       uint64_t max_legs, int32_t allow_contacts, double* out_positions, uint8_t* out_collided,
                                       uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags,
                                       uint32_t* out_choice, double* out_distance, uint32_t* out_legs_run);
/* Same with every pointer, the table's three included, in HBM (see fks_forward_simulate_device
 * for stream and synchronize): rows [a, b) with first_particle_id = a equal the same rows of the
 * whole call. */
fks_status fks_forward_simulate_policy_device(fks_context* ctx, const double* d_starts, uint64_t n, const fks_policy_table* table,
                                              uint64_t max_legs, uint64_t first_particle_id, int32_t allow_contacts,
                                              double* d_out_positions, uint8_t* d_out_collided, uint32_t* d_out_microsteps,
                                              uint32_t* d_out_resolver_iterations, uint32_t* d_out_error_flags,
                                              uint32_t* d_out_choice, double* d_out_distance, uint32_t* d_out_legs_run,
                                              void* stream, int32_t synchronize);

/* Outcome clustering (added within ABI 10): the planner's step after every forward batch.  G
 * groups of configurations go in, one group per job, as a batched call wrote them; each group's
 * configuration-distance matrix and its complete-link clusters under `threshold` come out.
 * group_begin holds G + 1 ascending offsets (in configurations) into configs [N][W], N =
 * group_begin[G]; group g is configurations [group_begin[g], group_begin[g + 1]), n of them.  The
 * configurations are taken as the bytes given: no ResetPosition, no clamping.
 *
 * Matrix of a group (row-major n x n doubles; the groups' matrices lie end to end, group g at the
 * sum of n_h^2 over h < g): for i < j, M[i][j] is the robot's configuration distance
 * (ComputeConfigurationDistanceTo) with cfg = c_i and target = c_j, in the arithmetic of the
 * kernels' distance (wrap of continuous dofs and of the SE(2) angle inside the difference, the
 * distance_weights, the SE(3) form through inverse / compose / log).  M[j][i] is the same bits:
 * mirrored, never computed as c_j -> c_i (the SE(3) distance is not bitwise symmetric).  M[i][i]
 * is +0.0.
 *
 * Clustering of a group: complete link, this library's statement (the planner's
 * arc_utilities/simple_hierarchical_clustering.hpp is not pinned against it).  For the clustering
 * only, a distance that is not < +inf (NaN, inf) counts as +inf.  Start with n singletons; a
 * cluster is named by its smallest member; the link of two clusters is L(a, b) = max of M[i][j]
 * over i in a, j in b.  Repeat: scan the live pairs (a, b), a < b, in ascending lexicographic
 * order and keep the smallest L under a strict < starting from +inf (the lowest pair wins a tie,
 * a +inf pair never wins); stop if no pair was kept or its L > threshold; otherwise merge b into a
 * (L <= threshold merges, equality included), with L(a u b, k) = max(L(a, k), L(b, k)), which is
 * exact.  The labels therefore depend on the matrix's bits and these rules alone.  Clusters are
 * numbered 0, 1, ... in ascending order of their smallest member: out_labels[i] (i an index into
 * configs) is its cluster's number within its group, out_num_clusters[g] the group's count (0 for
 * an empty group).  A negative threshold merges nothing, +inf merges every finite pair.
 *
 * out_distances, out_labels [N] and out_num_clusters [G] may each be NULL, not all three.  When
 * labels or counts are asked for, a group holds at most FKS_MAX_CLUSTER_GROUP configurations; with
 * both NULL only the matrices are made and that bound is lifted.  Refused with
 * FKS_ERR_INVALID_ARGUMENT, before anything is staged: a NaN threshold, all three outputs NULL,
 * 2^31 groups or more, NULL group_begin with G > 0, non-ascending offsets, N above 2^31, a
 * labelled group above the bound, a sum of n^2 above 2^27 doubles, NULL configs with N > 0, a
 * malformed robot (host twin); FKS_ERR_NO_ROBOT for a context without a robot.  The device entries
 * word every refusal in fks_get_last_error.  Empty groups and G == 0 succeed. */
#define FKS_MAX_CLUSTER_GROUP 256
/* The host twin: no context, no GPU.  The device entries below equal it byte for byte. */
fks_status fks_cluster_configs(const fks_robot_desc* robot, const double* configs, const uint64_t* group_begin,
                               uint64_t num_groups, double threshold, double* out_distances, uint32_t* out_labels,
                               uint32_t* out_num_clusters);
/* The same in one launch for the context's robot.  group_begin is a host array, staged by the
 * entry; every other pointer is in HBM (d_configs may be the output buffer of a batched call on
 * the same stream).  Stream and synchronize as fks_forward_simulate_device.  The call consumes no
 * call index and touches no statistics, work counters or last-call counters.  A working link
 * matrix of a group above 64 configurations lies in a workspace the context owns, grown on demand
 * and freed with the context. */
fks_status fks_cluster_configs_device(fks_context* ctx, const double* d_configs, const uint64_t* group_begin, uint64_t num_groups,
                                      double threshold, double* d_out_distances, uint32_t* d_out_labels,
                                      uint32_t* d_out_num_clusters, void* stream, int32_t synchronize);
/* The same on host buffers: one upload, one download per output array. */
fks_status fks_cluster_configs_ctx(fks_context* ctx, const double* configs, const uint64_t* group_begin, uint64_t num_groups,
                                   double threshold, double* out_distances, uint32_t* out_labels, uint32_t* out_num_clusters);

/* Cluster summaries (added within ABI 10): the planner's step after the clustering, every cluster
 * of every group made into a child state.  configs [N][W], group_begin [G + 1] (a host array) and
 * labels [N] are as a clustering call leaves them; targets [G][W], one per group, is optional and
 * goes with reached_distance.  The configurations are taken as the bytes given: no ResetPosition.
 *
 * Clusters and rows.  Cluster c of group g (n configurations) is {i : labels[i] == c} for c in
 * [0, n), whatever produced the labels: no density or ordering of the labels is assumed, and a
 * configuration whose label is >= n belongs to no cluster (none of the entries refuses it or
 * touches a row outside the group because of it).  Cluster c of group g owns row
 * r = group_begin[g] + c of every per-cluster output, so every such array has N rows, no prefix
 * over cluster counts exists and no count has to be downloaded to size a buffer.  Rows below
 * group_begin[0] belong to no group and are left as they are.
 *
 * Outputs (fks_cluster_summary: each pointer may be NULL, not all of them).
 *   order [N]         the stable regrouping: within group g, positions group_begin[g] ... hold the
 *                     indices into configs of cluster 0's members in ascending index, then cluster
 *                     1's, and so on; the configurations of no cluster come last, ascending.
 *   members [N][W]    members[k] = configs[order[k]], a byte copy: a cluster's members are
 *                     contiguous rows, fit to be the starts of a next fks_job.
 *   count [N]         the members of the row's cluster.
 *   begin [N]         the position in order / members of the cluster's first member; for an empty
 *                     cluster the position its first member would have (group_begin[g] + the
 *                     members of the group's clusters below c).
 *   expectation [N][W]
 *                     a limited dof (revolute, prismatic) and the SE(2) x, y: sum / count.  A
 *                     continuous dof and the SE(2) angle: atan2(sum of sin, sum of cos) in the
 *                     portable libm (fks_portable_math.h).  SE(3): entries 3, 7, 11 are sum / count;
 *                     the rotation block is that of the unit quaternion e which is the eigenvector
 *                     of the largest eigenvalue of S = sum of q q^T (Markley's mean; it does not
 *                     depend on the signs of the q), as stated below.
 *   variances [N][Wv] Wv = W (linked), 3 (SE(2)), 6 (SE(3)): sum of d^2 / count (the population
 *                     form), d the raw difference from the expectation to the member: c_i[k] - E[k],
 *                     through wrap_revolute for a continuous dof and the SE(2) angle; for SE(3) the
 *                     six components of log_twist34(compose34(inverse34(E), c_i)).
 *   variance [N]      sum of config_distance(cfg = E, target = c_i)^2 / count.
 *   reached [N]       only with targets: the members with config_distance(cfg = c_i, target =
 *                     targets[g]) < reached_distance, strict (SPCS:899); a NaN distance never counts.
 * Every sum over a cluster's members adds the terms (products and squares rounded first, no fused
 * multiply-add) one by one in ascending member index, starting from +0.0; host and device use this
 * one order, so the device entries equal the twin byte for byte.  The row of an empty cluster is
 * count 0, begin as stated, every double +0.0, reached 0.
 *
 * The rotation mean.  q = (w, x, y, z) of a member's rotation block R by Shepperd's rule: the
 * largest of (R00 + R11 + R22, R00, R11, R22), the lowest index winning a tie, names the component
 * c = sqrt(1 +- ...) / 2 taken from the diagonal; the other three are the matching sums or
 * differences of off-diagonal entries times 0.25 / c.  q is not normalised.  S's ten entries are
 * sums of the products q_a q_b.  Cyclic Jacobi on A = S, V = I: sweeps over (p, q) in the order
 * (0,1)(0,2)(0,3)(1,2)(1,3)(2,3), at most 16 sweeps.  At a pair: an A[p][q] that is zero is
 * passed; one with |A[p][q]| <= 2^-80 (A00 + A11 + A22 + A33), the trace taken before the first
 * sweep, is set to zero and passed; otherwise theta = (A[q][q] - A[p][p]) / (2 A[p][q]),
 * t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) (sign(0) = +1), c = 1 / sqrt(t^2 + 1), s = t c;
 * A[p][p] -= t A[p][q], A[q][q] += t A[p][q], A[p][q] = 0, and for the other rows r
 * (A[r][p], A[r][q]) <- (c A[r][p] - s A[r][q], s A[r][p] + c A[r][q]), mirrored; V's columns p
 * and q alike for every row.  The iteration stops after a sweep that rotated nothing, or at the
 * cap.  The eigenvector is V's column of the largest A[k][k], the lowest k winning a tie, divided
 * by its norm; the rotation block is 1 - 2 (yy + zz), 2 (xy - wz), ... of its components, every
 * entry a product of two of them.  Only + - * / and sqrt are used (csrc/fks_rotation_mean.h is the
 * one definition, shared by host and device).
 *
 * Parity with the planner's own averaging and variance code (uncertainty_planning_core,
 * arc_utilities) is not pinned: the entries are held to this statement and to nothing else.
 *
 * Limits and refusals.  A group holds at most FKS_MAX_CLUSTER_GROUP configurations, N is at most
 * 2^31, G is below 2^31.  Refused with FKS_ERR_INVALID_ARGUMENT before anything is staged: a NULL
 * summary or every output NULL, NULL group_begin with G > 0, non-ascending offsets, N above 2^31,
 * a group above the bound, NULL labels or configs with N > 0, reached without targets or targets
 * without reached, a NaN reached_distance when targets are given, a malformed robot (host twin);
 * FKS_ERR_NO_ROBOT for a context without a robot.  The device entries word every refusal in
 * fks_get_last_error.  Empty groups and G == 0 succeed. */
typedef struct fks_cluster_summary {
    uint32_t* order;     /* [N] */
    double* members;     /* [N][W] */
    uint32_t* count;     /* [N] */
    uint32_t* begin;     /* [N] */
    double* expectation; /* [N][W] */
    double* variances;   /* [N][Wv] */
    double* variance;    /* [N] */
    uint32_t* reached;   /* [N], with targets only */
} fks_cluster_summary;
/* The host twin: no context, no GPU.  The device entries below equal it byte for byte. */
fks_status fks_summarize_clusters(const fks_robot_desc* robot, const double* configs, const uint64_t* group_begin,
                                  uint64_t num_groups, const uint32_t* labels, const double* targets, double reached_distance,
                                  const fks_cluster_summary* out);
/* The same in one launch for the context's robot.  group_begin is a host array, staged by the
 * entry; d_configs, d_labels, d_targets and every pointer of d_out are in HBM (the summary struct
 * itself is a host struct).  Stream and synchronize as fks_forward_simulate_device.  The call
 * consumes no call index and touches no statistics, work counters or last-call counters.  The
 * per-member terms of the sums lie in a workspace the context owns, grown on demand and freed
 * with the context. */
fks_status fks_summarize_clusters_device(fks_context* ctx, const double* d_configs, const uint64_t* group_begin, uint64_t num_groups,
                                         const uint32_t* d_labels, const double* d_targets, double reached_distance,
                                         const fks_cluster_summary* d_out, void* stream, int32_t synchronize);
/* The same on host buffers: one upload, one download per output array. */
fks_status fks_summarize_clusters_ctx(fks_context* ctx, const double* configs, const uint64_t* group_begin, uint64_t num_groups,
                                      const uint32_t* labels, const double* targets, double reached_distance,
                                      const fks_cluster_summary* out);

/* State selection (added within ABI 10): the planner's step between a summary and the next jobs
 * call.  For each of J query configurations (the next sampled targets) the nearest state of a
 * resident table is chosen, and the state's member particles become the P starts of job j, written
 * where the next fks_job.starts reads them by device pointer; only the J indices have to come down.
 * A table is what successive summaries appended into one pool: keys are their `expectation` rows,
 * count and begin their `count` and `begin` (begin an absolute row of `members`).
 *
 * Selection of query q_j.  Configurations are taken as the bytes given: no ResetPosition, as in
 * clustering.  d_i = weights[i] * config_distance(cfg = keys[i], target = q_j), one rounded product
 * of the robot's configuration distance (config_distance_of<RT> on the device, fks_host_distance.h
 * on the host: the same expression trees over the portable libm).  With weights == NULL the product
 * is not formed, which equals all-1.0 weights bit for bit.  When count is given, a state with
 * count[i] == 0 is no state (the empty-cluster rows of a summary).  The choice is the i of the
 * smallest d_i under a strict < from +inf, scanned in ascending i: the lowest index wins a tie, a NaN
 * distance never wins and neither does a NaN weight.  No winner gives choice = FKS_STATE_NONE and
 * distance = +inf.  The caller folds the planner's feasibility and variance factors into weights.
 * Parity with uncertainty_planning_core's StateDistance is not pinned: the entries are held to this
 * statement and to nothing else.
 *
 * Draw of job j's starts, only when starts or source is asked for (it then needs P >= 1 and count,
 * begin, members).  Let c = count[choice], b = begin[choice].  If c == P, source[j][k] = b + k: no
 * draw, the members go over in order.  Otherwise source[j][k] = b + ((uint64_t)r_k * c >> 32), r_k
 * word k & 3 of Philox4x32-10 at the counter {low32(j), k >> 2, high32(j), 0x44524157} under the key
 * (k0, k1) = the low and high 32 bits of splitmix64(draw_seed) (x += 0x9E3779B97F4A7C15;
 * x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31).
 * Integer arithmetic only, so host and device agree by construction.  starts[j][k] is a byte copy
 * of members[source[j][k]].  Job j's rows are source = FKS_STATE_NONE and every double +0.0 when
 * the choice is FKS_STATE_NONE, or when b + c > num_member_rows (a guard against reading outside
 * the pool; choice and distance are still reported).  draw_seed is the caller's: the call consumes
 * no call index and moves no statistics, work counters or last-call counters.
 *
 * Limits and refusals.  S is 1 .. FKS_MAX_STATES, J at most 2^20, P at most 65,536, J x P at most
 * 2^31.  Refused with FKS_ERR_INVALID_ARGUMENT before anything is staged: a NULL table or
 * selection, NULL keys, S == 0 or above 2^30, NULL choice or queries with J > 0, starts or source
 * asked for with P == 0 or with count, begin or members NULL, begin without count, J above 2^20, P
 * above 65,536, J x P above 2^31, a malformed robot (host twin); FKS_ERR_NO_ROBOT for a context
 * without a robot.  The device entries word every refusal in fks_get_last_error.  J == 0 succeeds
 * and launches nothing. */
#define FKS_STATE_NONE 0xFFFFFFFFu
#define FKS_MAX_STATES (1ull << 30)
typedef struct fks_state_table {
    const double*   keys;      /* [S][W] the states' expectations (a summary's `expectation` rows) */
    const double*   weights;   /* [S], or NULL (= every weight 1.0) */
    const uint32_t* count;     /* [S] members of each state (a summary's `count`), or NULL */
    const uint32_t* begin;     /* [S] first member row in `members` (a summary's `begin`), or NULL */
    const double*   members;   /* [num_member_rows][W], or NULL */
    uint64_t num_states;       /* S, 1 .. 2^30 */
    uint64_t num_member_rows;
} fks_state_table;
typedef struct fks_state_selection {
    uint32_t* choice;    /* [J] required */
    double*   distance;  /* [J] may be NULL */
    double*   starts;    /* [J][P][W] may be NULL */
    uint32_t* source;    /* [J][P] may be NULL: the row of `members` each start is a copy of */
} fks_state_selection;
/* The host twin: no context, no GPU.  The device entries below equal it byte for byte. */
fks_status fks_select_states(const fks_robot_desc* robot, const fks_state_table* table, const double* queries, uint64_t num_queries,
                             uint32_t num_particles, uint64_t draw_seed, const fks_state_selection* out);
/* The same in two launches on the caller's stream for the context's robot: the two structs are host
 * structs, every pointer inside them and d_queries are in HBM.  Stream and synchronize as
 * fks_forward_simulate_device.  The partial results of the search lie in a workspace the context
 * owns, grown on demand and freed with the context. */
fks_status fks_select_states_device(fks_context* ctx, const fks_state_table* d_table, const double* d_queries, uint64_t num_queries,
                                    uint32_t num_particles, uint64_t draw_seed, const fks_state_selection* d_out, void* stream,
                                    int32_t synchronize);
/* The same on host buffers: one staged upload, one download per output array. */
fks_status fks_select_states_ctx(fks_context* ctx, const fks_state_table* table, const double* queries, uint64_t num_queries,
                                 uint32_t num_particles, uint64_t draw_seed, const fks_state_selection* out);
/* The decomposition a device call of J queries against S states takes on a device of
 * compute_units compute units (fks_batch::plan_select; no context, no GPU): out[0] queries per
 * workgroup, out[1] states per chunk, out[2] chunks per query, out[3] workgroups of the search. */
fks_status fks_select_states_plan(uint64_t num_queries, uint64_t num_states, int32_t compute_units, uint64_t out[4]);
/* Philox4x32-10 as the draw uses it (the host's own; for tests): counter and key in, four words out */
void fks_select_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);

/* CheckConfigCollision (SPCS:1398-1416) for a batch of n configurations (host
 * buffers): SetPosition(config), CheckEnvironmentCollision at threshold
 * inflation_ratio * res (SPCS:1403, 921-981) and CheckSelfCollisions at extended
 * cells of (inflation_ratio + 1) * res (SPCS:1404, 1324-1396).  out_collided[i] = 1
 * if configuration i collides; out_error_flags (may be NULL): FKS_PARTICLE_ERR_KEY_RANGE
 * for non-finite points.  The reference checks one configuration per call (the
 * planner's state-validity check); a batch of one is that call. */
fks_status fks_check_config_collision(fks_context* ctx, const double* configs, uint64_t n,
                                      double inflation_ratio, uint8_t* out_collided,
                                      uint32_t* out_error_flags);
/* Same with device buffers on the caller's stream (see fks_forward_simulate_device). */
fks_status fks_check_config_collision_device(fks_context* ctx, const double* d_configs, uint64_t n,
                                             double inflation_ratio, uint8_t* d_out_collided,
                                             uint32_t* d_out_error_flags, void* stream,
                                             int32_t synchronize);
/* counters of the last config-check call: particles = configurations, sdf_bytes,
 * kernel_ms, call_ms */
fks_status fks_get_last_check_counters(const fks_context* ctx, fks_call_counters* out);

/* ForwardSimulationStepTrace (simple_simulator_interface, filled at SPCS:1583-1595,
 * 1615-1618, 1701-1704, 1712-1715, 1776-1779) flattened per particle:
 *   resolver_steps[s].control_input / .control_input_step  -> step record s
 *   resolver_steps[s].contact_resolver_steps[m].contact_resolution_steps[k]
 *                                                          -> config records tagged (s, m, kind)
 * in the order the reference appends them.  Buffers are caller-owned, n particles x
 * capacity each; records beyond a capacity are counted but not stored. */
#define FKS_TRACE_POST_ACTION 0u    /* post_action_configuration of microstep m (SPCS:1617)          */
#define FKS_TRACE_RESOLVER_STEP 1u  /* active_configuration after a resolver iteration (SPCS:1703)  */
#define FKS_TRACE_RESOLVE_FAILED 2u /* previous_configuration, resolver gave up (SPCS:1714)         */
#define FKS_TRACE_CONTACT_STOP 3u   /* previous_configuration, contact with allow_contacts=false (SPCS:1778) */
typedef struct {
    uint32_t step_capacity;    /* step records per particle */
    uint32_t config_capacity;  /* configuration records per particle */
    double* step_inputs;       /* n * step_capacity * 2D: control_input (u * dt), control_input_step */
    uint32_t* step_microsteps; /* n * step_capacity: number of microsteps of the step */
    double* configs;           /* n * config_capacity * W */
    uint32_t* config_tags;     /* n * config_capacity * 3: controller step, microstep, FKS_TRACE_* kind */
    uint32_t* num_steps;       /* n: step records produced (may exceed step_capacity) */
    uint32_t* num_configs;     /* n: configuration records produced (may exceed config_capacity) */
} fks_trace;

/* ForwardSimulateRobot(..., trace, enable_tracing = true, ...) (SPCS:824-829) for a
 * batch: same results as fks_forward_simulate plus the trace of every particle
 * (host buffers; the traced kernel is a separate instantiation, the untraced path
 * does not pay for it). */
fks_status fks_forward_simulate_traced(fks_context* ctx, const double* starts, uint64_t n,
                                       const double* targets, uint64_t num_targets,
                                       int32_t allow_contacts, double* out_positions,
                                       uint8_t* out_collided, uint32_t* out_microsteps,
                                       uint32_t* out_resolver_iterations, uint32_t* out_error_flags,
                                       const fks_trace* trace);

/* ForwardSimulateMutableRobot(..., trace, enable_tracing = true, ...) (SPCS:843-919) for a
 * batch: fks_forward_simulate_mutable's controller state in/out plus the trace. */
fks_status fks_forward_simulate_traced_mutable(fks_context* ctx, const double* starts, uint64_t n, const double* targets,
                                               uint64_t num_targets, int32_t allow_contacts, double* controller_state,
                                               double* out_positions, uint8_t* out_collided, uint32_t* out_microsteps,
                                               uint32_t* out_resolver_iterations, uint32_t* out_error_flags,
                                               const fks_trace* trace);

/* Kinematics of a batch of configurations (host buffers), the pieces the reference's
 * host-side helpers build on, computed with the simulation kernels' own FK:
 *   FKS_KIN_LINK_TRANSFORMS     out: n x num_links x 12 (3x4 row-major link transforms
 *                               after SetPosition; GetLinkTransform, used by
 *                               Get3dPointForConfig SPCS:776-786)
 *   FKS_KIN_POINTS              out: n x num_points x 3 (link points in the world frame,
 *                               geometry order; MakeConfigurationDisplayRep SPCS:634-688)
 *   FKS_KIN_APPLY_CONTROL_INPUT inputs: n x num_dofs; out: n x config width (the clean
 *                               ApplyControlInput of MakeControlInputDisplayRep,
 *                               SPCS:719-774, TNUVA:538-566) */
#define FKS_KIN_LINK_TRANSFORMS 0
#define FKS_KIN_POINTS 1
#define FKS_KIN_APPLY_CONTROL_INPUT 2
fks_status fks_kinematics(fks_context* ctx, int32_t mode, const double* configs, uint64_t n, const double* inputs,
                          double* out);
/* sizes of the robot set with fks_set_robot (any pointer may be NULL) */
fks_status fks_robot_sizes(const fks_context* ctx, int32_t* num_links, int32_t* num_points, int32_t* num_dofs,
                           int32_t* config_width);

/* Each forward/reverse call consumes one RNG "call index" (the reference's
 * per-thread std::mt19937_64 streams advance across calls, SPCS:850).  Ranks
 * that shard one logical call must use the same index: set it explicitly. */
fks_status fks_set_call_index(fks_context* ctx, uint64_t call_index);
uint64_t fks_get_call_index(const fks_context* ctx);

fks_status fks_get_statistics(const fks_context* ctx, fks_statistics* out);
fks_status fks_reset_statistics(fks_context* ctx);
/* overwrite the statistics (a caller that re-runs a call restores what it read before) */
fks_status fks_set_statistics(fks_context* ctx, const fks_statistics* stats);
fks_status fks_reset_generators(fks_context* ctx, uint64_t prng_seed);
int32_t fks_get_debug_level(const fks_context* ctx);
int32_t fks_set_debug_level(fks_context* ctx, int32_t debug_level);
fks_status fks_get_last_call_counters(const fks_context* ctx, fks_call_counters* out);
/* Kernel phase profile: shader-clock cycles (s_memtime) spent by all waves in each
 * phase of the hot path, summed over the particles of a call.  Diagnostic only;
 * the phases follow the reference's call structure (SPCS line ranges). */
#define FKS_NUM_PHASES 16
enum fks_phase {
    FKS_PHASE_PARTICLE = 0,        /* whole particle: ForwardSimulateMutableRobot SPCS:843-919 */
    FKS_PHASE_CONTROL = 1,         /* controller + sensor noise SPCS:861-876 */
    FKS_PHASE_STEP_SETUP = 2,      /* microstep count estimate SPCS:1549-1572 */
    FKS_PHASE_MICRO_INPUT = 3,     /* ApplyControlInput incl. actuator noise SPCS:1599, TNUVA:568-596 */
    FKS_PHASE_MICRO_FK = 4,        /* SetPosition (FK) of the post-action configuration SPCS:1600-1601 */
    FKS_PHASE_ENV_CHECK = 5,       /* CheckEnvironmentCollision SPCS:921-981 */
    FKS_PHASE_SELF_CHECK = 6,      /* CollectSelfCollisions SPCS:1183-1275 (+ ExtractSelfCollidingPoints 983-1171) */
    FKS_PHASE_CORRECTIONS = 7,     /* CollectPointCorrectionsAndJacobians SPCS:1818-1939 */
    FKS_PHASE_SOLVE = 8,           /* ComputeResolverCorrectionStep{StackedJacobian,IndividualJacobians} SPCS:1966-1998 */
    FKS_PHASE_RESOLVE_APPLY = 9,   /* correction step sizing / application SPCS:1630-1690 */
    FKS_PHASE_OUTPUT = 10,         /* reached configuration + counters */
    /* event counts (not cycles) of the profiling build */
    FKS_PHASE_ENV_ROUNDS_SKIPPED = 11,   /* 64-point rounds proven free (no SDF reads) */
    FKS_PHASE_ENV_ROUNDS_EVALUATED = 12, /* 64-point rounds read from the SDF */
    FKS_PHASE_CORR_ROUNDS_SKIPPED = 13,  /* correction rounds proven free */
    FKS_PHASE_CORR_ROUNDS_EVALUATED = 14,
    /* residency of the persistent waves: 100 MHz s_memrealtime ticks from a wave's
     * start to its exit (queue drained), summed over waves; with the kernel time it
     * gives the share of wave slots kept busy (the batch's tail) */
    FKS_PHASE_WAVE_RESIDENCY = 15
};
/* which: 0 = last call, 1 = sums since fks_create / fks_reset_total_counters */
fks_status fks_get_phase_cycles(const fks_context* ctx, int which, uint64_t* out /* FKS_NUM_PHASES */);
/* Launch geometry of the simulation kernel for the robot set last: resident waves of
 * the persistent grid (CUs x workgroups per CU x waves per workgroup, one particle
 * per wave at a time) and LDS bytes per workgroup.  Diagnostic (no reference
 * counterpart); with FKS_PHASE_WAVE_RESIDENCY it gives the busy share of the grid. */
fks_status fks_get_launch_geometry(const fks_context* ctx, uint32_t* resident_waves, uint64_t* lds_bytes_per_group);
/* which simulation kernel a call ran (fks_launch_info.last_kernel) */
typedef enum {
    FKS_KERNEL_NONE = 0,
    FKS_KERNEL_THROUGHPUT = 1,   /* fks_simulate_<family>[_lean] */
    FKS_KERNEL_SMALL_BATCH = 2,  /* fks_simulate_<family>_small (fks_set_small_batch_kernel) */
    FKS_KERNEL_SHAPED = 3,       /* the robot-shape-specialised kernel (fks_set_specialization) */
    FKS_KERNEL_TRACED = 4,       /* fks_simulate_<family>[_lean]_traced */
    FKS_KERNEL_INDIVIDUAL = 5,   /* fks_simulate_<family>[_lean]_indiv (fks_set_individual_jacobians) */
    FKS_KERNEL_COOPERATIVE = 6,  /* ABI 10: fks_simulate_<family>_coop (fks_set_cooperative_waves) */
    FKS_KERNEL_SHAPED_SMALL_BATCH = 7, /* ABI 10: the shape-specialised module's small-batch kernel
                                          (a small batch once the robot's module is built) */
    FKS_KERNEL_PATH = 8,             /* fks_simulate_<family>[_lean]_path (fks_forward_simulate_path) */
    FKS_KERNEL_PATH_SMALL_BATCH = 9, /* fks_simulate_<family>_path_small: a path whose batch fits the
                                        small-batch kernel's resident waves */
    FKS_KERNEL_JOBS = 10,            /* fks_simulate_<family>[_lean]_jobs (fks_forward_simulate_jobs) */
    FKS_KERNEL_JOBS_SMALL_BATCH = 11, /* fks_simulate_<family>_jobs_small: a job batch whose particles
                                         together fit the small-batch kernel's resident waves */
    FKS_KERNEL_PATH_JOBS = 12,        /* fks_simulate_<family>[_lean]_path_jobs (fks_forward_simulate_path_jobs) */
    FKS_KERNEL_PATH_JOBS_SMALL_BATCH = 13, /* fks_simulate_<family>_path_jobs_small: a path-job batch whose
                                              particles together fit the small-batch kernel's resident waves */
    FKS_KERNEL_SHAPED_PATH_JOBS = 14,      /* fks_simulate_shaped_pj of the robot's batched module: a path, job
                                              or path-job batch (fks_prepare_batched_specialization) */
    FKS_KERNEL_SHAPED_PATH_JOBS_SMALL_BATCH = 15, /* fks_simulate_shaped_pj_small: such a batch within the
                                                     small-batch kernel's resident waves, once the module is built */
    FKS_KERNEL_POLICY = 16,            /* fks_simulate_<family>[_lean]_policy (fks_forward_simulate_policy) */
    FKS_KERNEL_POLICY_SMALL_BATCH = 17 /* fks_simulate_<family>_policy_small: a roll-out whose batch fits the
                                          small-batch kernel's resident waves */
} fks_kernel_kind;
/* The launch layout fks_set_robot chose (ABI 8; diagnostic, no reference counterpart). */
typedef struct fks_launch_info {
    uint32_t resident_waves;                 /* the persistent grid (fks_get_launch_geometry) */
    uint32_t waves_per_group;
    uint64_t lds_bytes_per_group;
    uint32_t small_batch_resident_waves;     /* the small-batch kernel's grid (0: not for this layout) */
    uint32_t standard_layout_resident_waves; /* what the non-lean LDS layout would hold */
    int32_t fk_pair;                         /* paired FK of free microsteps */
    int32_t lean;                            /* lean LDS block (skip-proof cache in scratch) */
    int32_t last_kernel;                     /* fks_kernel_kind of the last simulation call */
    int32_t last_check_kernel;               /* ABI 9: of the last batched CheckConfigCollision call
                                                (FKS_KERNEL_THROUGHPUT: generic, FKS_KERNEL_SHAPED) */
    uint32_t cooperative_resident_particles; /* ABI 10: the cooperative kernel's grid (0: not for this robot) */
    uint32_t cooperative_waves_per_particle; /* ABI 10: its waves per particle (workgroup) */
} fks_launch_info;
fks_status fks_get_launch_info(const fks_context* ctx, fks_launch_info* out);
/* Scheduling granularity of fks_forward_simulate*: when a batch holds more particles
 * than the grid has resident waves, each particle's controller steps are run in
 * segments of `controller_steps` (0 = automatic: 14 when the batch outnumbers the
 * resident waves, else whole; nonzero: always), handed out segment-major so
 * that every particle progresses from the start of the launch and contact-heavy
 * particles do not start last (the batch's tail).  Results are bit-identical for
 * every value (the resting state between segments is exact).  No reference
 * counterpart (SPCS:795 runs each particle whole on one OpenMP thread). */
fks_status fks_set_segment_steps(fks_context* ctx, uint32_t controller_steps);
/* Scheduling policy of segmented batches (ABI 3; no reference counterpart, results are
 * bit-identical for every value):
 *   heavy_resolver_per_step: a segment whose particle averaged at least this many
 *     resolver iterations per controller step is contact-heavy and its wave keeps the
 *     particle's next segment instead of returning it to the round-robin (0 = off;
 *     default 2; at most 65536);
 *   heavy_priority: issue priority (s_setprio 0..2) of a wave carrying a contact-heavy
 *     particle (1 = raised to 2 for heavy segments only; 0 = never raised; 2, the default
 *     since ABI 10 = also 1 for particles that fell behind the round-robin).
 * The priority is reset to 0 at the start of every segment a wave claims. */
fks_status fks_set_segment_policy(fks_context* ctx, uint32_t heavy_resolver_per_step, uint32_t heavy_priority);
/* ABI 10: once the batch's mean resolver iterations per finished segment reaches the absolute
 * threshold (a contact-heavy batch), a heavy segment must also have at least `times_mean` times
 * that mean (the kernel keeps the running sums; default 3, 0 = the absolute test alone, at most
 * 64; off for batches of 2^24 or more particle-segments).  Results are bit-identical for every
 * value. */
fks_status fks_set_segment_heavy_relative(fks_context* ctx, uint32_t times_mean);
/* Small batches (ABI 7; no reference counterpart, results are bit-identical either way):
 * with `enabled` (the default) a plain simulation call whose particles all fit the
 * resident waves of a low-occupancy instantiation (two waves per SIMD, no register
 * spills; not for lean LDS blocks, traced or individual-Jacobian calls, or explicit
 * segments) runs that kernel — a batch that small is the latency of its slowest particle
 * (a planner's typical call: cfg1, 32 particles, 10 % shorter).  0 = always the
 * throughput kernel. */
fks_status fks_set_small_batch_kernel(fks_context* ctx, int32_t enabled);
/* Cooperative small batches (ABI 10; no reference counterpart, results are bit-identical
 * either way; opt-in, default 0): with `enabled` a plain simulation call of at most
 * fks_launch_info.cooperative_resident_particles particles (one per workgroup slot: 256 CUs
 * x the kernel's occupancy; same exclusions as the small-batch kernel, robots of at most
 * 1024 points) runs each particle on a workgroup of cooperative_waves_per_particle waves: one
 * runs the particle, and every environment check and correction pass is shared out over all
 * of them, 64-point rounds each.  Takes precedence over the small-batch kernel;
 * fks_set_small_batch_kernel(ctx, 0) turns both off.  Measured on cfg3's heaviest particles
 * alone it is 5-10 % SLOWER than the small-batch kernel (about three rounds per check are left
 * after the skip proofs, too few to share), hence off by default. */
fks_status fks_set_cooperative_waves(fks_context* ctx, int32_t enabled);
/* SimpleParticleContactSimulator(..., simulate_with_individual_jacobians, ...) (SPCS:420-423,
 * 1629): 0 = ComputeResolverCorrectionStepStackedJacobian (SPCS:1990-1998; what the factories
 * FKS.cpp:22,45,68 hard-wire, the default), 1 = ComputeResolverCorrectionStepIndividualJacobians
 * (SPCS:1966-1988: one ColPivHouseholderQR solve per corrected point, summed in point order). */
fks_status fks_set_individual_jacobians(fks_context* ctx, int32_t simulate_with_individual_jacobians);
/* Robot-shape specialisation (ABI 8; no reference counterpart, results are bit-identical
 * either way).  While enabled (the default), the plain throughput simulation
 * (fks_forward_simulate*, not traced, individual-Jacobian or small-batch calls) runs a kernel
 * compiled at run time (hiprtc, in the helper process fks_shapec installed beside the
 * library) from the library's own kernel source with the robot's link / joint / dof /
 * geometry counts and LDS and scratch carve-outs as constants (cfg3: 10-13 % faster,
 * DESIGN.md §4.9).  A robot's kernel is built at the first call that runs it (a robot only
 * simulated in small batches never compiles) or at once by fks_set_specialization(ctx, 1);
 * the first robot of a shape on a machine costs one compile (2-20 s in the calling thread),
 * later ones come from the per-process cache or the disk cache (FKS_KERNEL_CACHE=<dir>,
 * default ~/.cache/fast_kinematic_simulator_amd; "off" disables it).  When the kernel cannot
 * be built the calls keep the generic kernel (same results), fks_get_specialization reports
 * failed = 1 with the compiler log in `message`, and so does fks_get_last_error;
 * fks_set_specialization(ctx, FKS_SPECIALIZE_ON) then returns FKS_ERR_UNSUPPORTED.
 * FKS_SPECIALIZE_OFF = generic kernels only (also the default when the environment variable
 * FKS_SPECIALIZE=0 is set at fks_create).  FKS_SPECIALIZE_NO_PROOFS (ABI 9, validation only)
 * builds the same shaped kernel with every skip proof compiled out (FKS_NO_SKIP_PROOFS: the
 * environment / correction round proofs, the motion-estimate pruning, the self-collision gap
 * proof and both lever-arm shortcuts): the results must not change, only the
 * time, which is what tests/test_proof_free.py checks on full batches. */
typedef enum {
    FKS_SPECIALIZE_OFF = 0,
    FKS_SPECIALIZE_ON = 1,
    FKS_SPECIALIZE_NO_PROOFS = 2
} fks_specialization_mode;
fks_status fks_set_specialization(fks_context* ctx, int32_t mode);
typedef struct fks_specialization_info {
    int32_t enabled;         /* fks_set_specialization's mode (fks_specialization_mode) */
    int32_t active;          /* the current robot's plain simulation calls run the shape-specialised kernel */
    int32_t from_cache;      /* its code object came from the process or disk cache */
    int32_t pending;         /* enabled, robot set, kernel to be built at the first call that runs it */
    double compile_seconds;  /* hiprtc time of that code object (0 when it came from a cache) */
    uint64_t launches;       /* launches of the specialised kernel since the robot was set */
    char shape[64];          /* the shape key, e.g. "t0-L8-J7-D7-W7-G8-P512-p1-l0" */
    int32_t failed;          /* ABI 9: the current robot's build failed; its calls run the generic kernel */
    int32_t reserved;
    char message[512];       /* ABI 9: why it failed (the start of the compiler log), else empty */
} fks_specialization_info;
fks_status fks_get_specialization(const fks_context* ctx, fks_specialization_info* out);
/* The batched module (added within ABI 10): the same robot shape's kernels for path, job and
 * path-job batches (fks_forward_simulate_path / _jobs / _path_jobs and their _device forms), in
 * a code object of its own whose shape key ends in "-b".  It is opt-in: a context keeps its
 * batches on the generic kernels until fks_set_batched_specialization(ctx, 1) or
 * fks_prepare_batched_specialization.  Once enabled, and with fks_set_specialization at
 * FKS_SPECIALIZE_ON (OFF and NO_PROOFS keep batches on the generic kernels), it is built, or
 * fetched from the caches above, at the first batch that runs its throughput kernel (more
 * particles than small_batch_resident_waves, or segments set), or at once by
 * fks_prepare_batched_specialization, which also enables it and returns FKS_ERR_UNSUPPORTED
 * with the log when the build fails; fks_set_specialization itself builds only the plain
 * module, and releases this one (built again at the next such batch).  A batch that fits
 * the small-batch grid never builds it and runs the module's small-batch kernel only once the
 * module exists (never on a lean block).  A failed build leaves the generic batched kernels in
 * place (same results), sets failed / message here and adds to fks_get_last_error without
 * failing the call.  All three entries then report FKS_KERNEL_SHAPED_PATH_JOBS[_SMALL_BATCH]:
 * one PATH-and-JOBS kernel serves them (a path is one path job, a job a path job of one leg;
 * a path of more than FKS_MAX_PATH_JOB_LEGS legs keeps the generic path kernel).  Results,
 * statistics, counters and call indices are those of the generic kernels.
 * fks_set_batched_specialization(ctx, 0), the default, keeps batches generic while plain calls
 * stay shaped; a module already built is kept.  fks_get_batched_specialization fills the
 * plain module's struct for this one (`enabled` is fks_set_batched_specialization's value,
 * `pending` is set only while enabled). */
fks_status fks_prepare_batched_specialization(fks_context* ctx);
fks_status fks_set_batched_specialization(fks_context* ctx, int32_t enabled);
fks_status fks_get_batched_specialization(const fks_context* ctx, fks_specialization_info* out);

/* sums over every call since fks_create / fks_reset_total_counters */
fks_status fks_get_total_counters(const fks_context* ctx, fks_call_counters* out);
fks_status fks_reset_total_counters(fks_context* ctx);
fks_status fks_set_total_counters(fks_context* ctx, const fks_call_counters* totals);

/* One robot stepped by hand on the host (the TnuvaRobot control interface, TNUVA:15-23), the
 * same arithmetic as the simulation kernels:
 *   fks_robot_control_action       -> GenerateControlAction(target, controller_interval)
 *                                     (TNUVA:179-198, 384-412, 598-614); pid_state: the robot's
 *                                     controllers, 2 * num_dofs doubles (error integrals, then
 *                                     last errors), updated in place; out_control: num_dofs
 *   fks_robot_apply_control_input  -> ApplyControlInput(u) (TNUVA:152-163, 348-364, 538-566)
 *                                     with unit_noise NULL; ApplyControlInput(u, rng)
 *                                     (TNUVA:165-177, 366-382, 568-596) with one truncated-normal
 *                                     TN(0, 0.5) on [-1, 1] sample per dof drawn by the caller
 *                                     (UNC:77-90); out_config: the robot's config width */
fks_status fks_robot_control_action(const fks_robot_desc* robot, const double* config, const double* target,
                                    double controller_interval, double* pid_state, double* out_control);
fks_status fks_robot_apply_control_input(const fks_robot_desc* robot, const double* config, const double* input,
                                         const double* unit_noise, double* out_config);

/* ---- environment preprocessing (CPU; reference SEB.cpp:21-476) ---- */
/* OBSTACLE_CONFIG (SEB.hpp): pose as 3x4 row-major, half extents, object id > 0 */
typedef struct {
    double pose[12];
    double extents[3];
    uint32_t object_id;
    uint32_t reserved;
} fks_obstacle;

typedef struct fks_env_handle fks_env_handle;

/* BuildCompleteEnvironment(obstacles, resolution).  If `grid_origin` and
 * `num_cells` are non-NULL the grid is that box (a fixed-size grid, e.g. 256^3);
 * otherwise it is sized to the obstacles plus a 3-cell border (SEB.cpp:128-149). */
fks_status fks_env_build(const fks_obstacle* obstacles, int32_t num_obstacles,
                         double resolution, const double* grid_origin,
                         const int64_t* num_cells, fks_env_handle** out);
/* The same environment built on the GPU (obstacle rasterisation, exact squared EDT,
 * surface-normal CSR: fks_env_gpu.hip); bit-identical to fks_env_build.  The result
 * is copied back into a host handle (fks_env_view / fks_env_free as above).
 * stats (optional): sizes and the device time of the build. */
typedef struct {
    uint64_t cells;
    uint64_t obstacle_samples;
    uint64_t normal_entries;
    double gpu_ms;   /* device time: rasterise + EDT + SDF + CSR (HIP events) */
    double total_ms; /* host wall time of the call incl. allocation and copy-back */
} fks_env_build_stats;
fks_status fks_env_build_gpu(const fks_obstacle* obstacles, int32_t num_obstacles,
                             double resolution, const double* grid_origin,
                             const int64_t* num_cells, int32_t device, fks_env_handle** out,
                             fks_env_build_stats* stats);
/* The same GPU build kept in device memory, handed to a context without a trip
 * through the host (the simulation reads exactly these bytes). */
typedef struct fks_device_env fks_device_env;
fks_status fks_env_build_device(const fks_obstacle* obstacles, int32_t num_obstacles,
                                double resolution, const double* grid_origin,
                                const int64_t* num_cells, int32_t device, fks_device_env** out,
                                fks_env_build_stats* stats);
/* host copy of a device environment (then fks_env_view / fks_env_occupancy / fks_env_free) */
fks_status fks_device_env_download(const fks_device_env* env, fks_env_handle** out);
fks_status fks_device_env_geometry(const fks_device_env* env, fks_grid_geometry* out);
void fks_device_env_free(fks_device_env* env);
/* fks_create on the device environment's own device: the SDF and surface-normal CSR are
 * copied device to device; the context does not keep a reference to `env`. */
fks_status fks_create_from_device_env(const fks_device_env* env, const fks_solver_params* params,
                                      double simulation_controller_frequency, uint64_t prng_seed,
                                      int32_t debug_level, fks_context** out_ctx);
/* DiscretizeObstacle (SEB.cpp:21-46): *count = the obstacle's half-resolution samples; with
 * out_xyz (capacity >= *count triples) their positions relative to the obstacle (its frame: the
 * caller places them with obstacle.pose, as BuildEnvironment does, SEB.cpp:84-85), x then y
 * then z */
fks_status fks_env_discretize_obstacle(const fks_obstacle* obstacle, double resolution, double* out_xyz, uint64_t capacity,
                                       uint64_t* count);
/* BuildSurfaceNormalsGrid (SEB.cpp:258-468) on the caller's SDF (VoxelGrid order over
 * sdf_geometry, e.g. sdf_tools' ExtractSignedDistanceField result, SEB.cpp:473-475): a handle
 * with only the surface-normal CSR over that geometry (fks_env_view: sdf_values NULL) */
fks_status fks_env_build_normals(const fks_obstacle* obstacles, int32_t num_obstacles, const fks_grid_geometry* sdf_geometry,
                                 const float* sdf_values, fks_env_handle** out);
/* the object id of each cell of an fks_env_build collision map (BuildEnvironment's
 * SetValue(1.0, object_id) in obstacle order, the last write wins, SEB.cpp:151-155; 0 = free) */
fks_status fks_env_cell_objects(const fks_env_handle* env, uint32_t* out, uint64_t num_cells);

/* Fill a view whose pointers stay valid until fks_env_free. */
fks_status fks_env_view(const fks_env_handle* env, fks_environment* out);
/* The collision grid (1 = filled cell), z-fastest, num_cells = nx * ny * nz. */
fks_status fks_env_occupancy(const fks_env_handle* env, uint8_t* out, uint64_t num_cells);
void fks_env_free(fks_env_handle* env);

/* ---- several devices in one process (fks_multi.cpp) ----
 * The reference runs one simulator object over all host cores (`#pragma omp parallel for`
 * over particles, SPCS:795); a multi context runs one fks_context per listed device and
 * splits every batch into contiguous shards, particle i on the device whose
 * fks_shard_bounds range holds it, simulated with first_particle_id = the range start
 * (bit-identical results for any device list).  Each device has a host thread of its own for
 * the call: it stages its shard through pinned buffers of its own (H2D, kernel, D2H on the
 * device's stream, so no device's copies wait for another's), and copies its outcomes into
 * the caller's buffers at its offset; statistics and call counters are summed over the
 * devices (kernel_ms: the slowest).  The same device may be listed more than once. */
typedef struct fks_multi_context fks_multi_context;
/* [begin, end) of shard `shard` of n particles over ndev devices: balanced contiguous ranges,
 * the first n % ndev shards one particle longer */
fks_status fks_shard_bounds(uint64_t n, int32_t ndev, int32_t shard, uint64_t* begin, uint64_t* end);
fks_status fks_create_multi(const fks_environment* env, const fks_solver_params* params, double simulation_controller_frequency,
                            uint64_t prng_seed, int32_t debug_level, const int32_t* devices, int32_t ndev,
                            fks_multi_context** out);
void fks_destroy_multi(fks_multi_context* m);
const char* fks_multi_get_last_error(const fks_multi_context* m);
int32_t fks_multi_num_devices(const fks_multi_context* m);
/* the per-device context of shard `shard` (for per-device settings such as fks_set_segment_steps) */
fks_context* fks_multi_device_context(fks_multi_context* m, int32_t shard);
fks_status fks_multi_set_robot(fks_multi_context* m, const fks_robot_desc* robot);
/* ABI 9: the batches that follow are sharded over the first `count` listed devices only
 * (1 <= count <= fks_multi_num_devices; 0 = all).  A batch too small to keep every device
 * busy for longer than its slowest particle runs no faster on more devices, so
 * the planner-facing DeviceSet picks the count per batch from the particles per device. */
fks_status fks_multi_set_active_devices(fks_multi_context* m, int32_t count);
int32_t fks_multi_active_devices(const fks_multi_context* m);
/* ForwardSimulateRobots (SPCS:788-804) over the active devices; arguments as fks_forward_simulate */
fks_status fks_multi_forward_simulate(fks_multi_context* m, const double* starts, uint64_t n, const double* targets,
                                      uint64_t num_targets, int32_t allow_contacts, double* out_positions, uint8_t* out_collided,
                                      uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags);
/* fks_forward_simulate_path over the active devices: the same contiguous shards, every shard at
 * the multi context's call index, which then advances by num_legs */
fks_status fks_multi_forward_simulate_path(fks_multi_context* m, const double* starts, uint64_t n, const double* waypoints,
                                           uint64_t num_legs, uint64_t num_targets, int32_t allow_contacts, double* out_positions,
                                           uint8_t* out_collided, uint32_t* out_microsteps, uint32_t* out_resolver_iterations,
                                           uint32_t* out_error_flags);
/* fks_forward_simulate_jobs over the active devices: the jobs' particles laid end to end are cut
 * into the same contiguous shards; a device gets, of every job its shard meets, the sub-range
 * with first_particle_id = the sub-range's start within the job, and every other job empty, so
 * every device consumes num_jobs call indices from the multi context's, which then advances by
 * num_jobs.  Refusals as fks_forward_simulate_jobs */
fks_status fks_multi_forward_simulate_jobs(fks_multi_context* m, const fks_job* jobs, uint64_t num_jobs);
/* fks_forward_simulate_path_jobs over the active devices, cut in the same way: of every job its
 * shard meets a device gets the sub-range (its rows of every leg), and every other job empty
 * with its num_legs kept, so all devices consume the same sum of num_legs call indices. */
fks_status fks_multi_forward_simulate_path_jobs(fks_multi_context* m, const fks_path_job* jobs, uint64_t num_jobs);
fks_status fks_multi_get_statistics(const fks_multi_context* m, fks_statistics* out);
fks_status fks_multi_reset_statistics(fks_multi_context* m);
fks_status fks_multi_get_last_call_counters(const fks_multi_context* m, fks_call_counters* out);
fks_status fks_multi_set_call_index(fks_multi_context* m, uint64_t call_index);
/* Batched CheckConfigCollision (SPCS:1398-1416) over all devices: configuration i on the
 * device whose fks_shard_bounds range holds it; arguments as fks_check_config_collision. */
fks_status fks_multi_check_config_collision(fks_multi_context* m, const double* configs, uint64_t n, double inflation_ratio,
                                            uint8_t* out_collided, uint32_t* out_error_flags);
/* Number of MI355X devices visible to this process (HIP_VISIBLE_DEVICES applies); 0 when there
 * is none.  The planner-facing factories default to all of them (fast_kinematic_simulator.hpp). */
int32_t fks_device_count(void);

/* Device self-test of the portable libm against the host (bit equality). */
fks_status fks_selftest_math(int32_t device, uint64_t n, uint64_t* out_mismatches);

#ifdef __cplusplus
}
#endif

#endif /* FKS_CAPI_H */
