/*
 * fks_kernel_list.h — every generic kernel that takes a SimArgs, named once:
 *   FKS_KERNEL(symbol, attributes, entry, flavour, form, budget, family)
 *   FKS_POLICY_KERNEL(...)    the same columns; the kernel takes the call's PolicyArgs second
 * attributes: THROUGHPUT, SMALL or COOPERATIVE (launch bounds and waves per SIMD, fks_kernels.hip).
 * entry: the template the kernel instantiates (simulate_particles, check_configs, kinematics).
 * flavour: simulate_particles' template arguments by name, or'ed (F_NONE: none).
 * form, budget, family: the kernel's identity (fks_launch.h); the robot type is the family's.
 *
 * Included with the two macros defined, once per expansion, and undefines them: fks_kernels.hip
 * makes the definitions of it, in this order, fks_capi.cpp the declarations and the function
 * pointers, fks_launch.cpp the identities and symbol names (kernel_row resolves an identity that
 * has no row).  A shape-specialised build never opens this file.
 */

/* one kernel per robot family so each carries only its own FK / Jacobian code */
FKS_KERNEL(fks_simulate_linked, THROUGHPUT, simulate_particles, F_NONE, PLAIN, THROUGHPUT, LINKED)
FKS_KERNEL(fks_simulate_se2, THROUGHPUT, simulate_particles, F_NONE, PLAIN, THROUGHPUT, SE2)
FKS_KERNEL(fks_simulate_se3, THROUGHPUT, simulate_particles, F_NONE, PLAIN, THROUGHPUT, SE3)

/* small batches (fks_set_small_batch_kernel): at most two waves per SIMD, so the register
 * budget holds the whole working set without spills.  One particle per wave and no
 * segments, chosen only when the batch fits its resident waves: such a batch is the
 * latency of its slowest particle, not a throughput problem (cfg1: 3.8-3.9 ms against
 * 4.2-4.35, profiles/r04j_occupancy_ab_cfg1.log). */
FKS_KERNEL(fks_simulate_linked_small, SMALL, simulate_particles, F_NONE, PLAIN, SMALL, LINKED)
FKS_KERNEL(fks_simulate_se2_small, SMALL, simulate_particles, F_NONE, PLAIN, SMALL, SE2)
FKS_KERNEL(fks_simulate_se3_small, SMALL, simulate_particles, F_NONE, PLAIN, SMALL, SE3)

/* cooperative small batches (fks_set_cooperative_waves): one particle per workgroup of
 * FKS_COOP_WAVES waves, whose environment checks and correction passes are shared out over
 * them; for batches up to one particle per workgroup slot */
FKS_KERNEL(fks_simulate_linked_coop, COOPERATIVE, simulate_particles, F_COOP, COOPERATIVE, THROUGHPUT, LINKED)
FKS_KERNEL(fks_simulate_se2_coop, COOPERATIVE, simulate_particles, F_COOP, COOPERATIVE, THROUGHPUT, SE2)
FKS_KERNEL(fks_simulate_se3_coop, COOPERATIVE, simulate_particles, F_COOP, COOPERATIVE, THROUGHPUT, SE3)

/* simulate_with_individual_jacobians = true (SPCS:420, 1629; fks_set_individual_jacobians) */
FKS_KERNEL(fks_simulate_linked_indiv, THROUGHPUT, simulate_particles, F_INDIVIDUAL, INDIVIDUAL, THROUGHPUT, LINKED)
FKS_KERNEL(fks_simulate_se2_indiv, THROUGHPUT, simulate_particles, F_INDIVIDUAL, INDIVIDUAL, THROUGHPUT, SE2)
FKS_KERNEL(fks_simulate_se3_indiv, THROUGHPUT, simulate_particles, F_INDIVIDUAL, INDIVIDUAL, THROUGHPUT, SE3)

/* traced instantiations: ForwardSimulateRobot with enable_tracing (fks_forward_simulate_traced) */
FKS_KERNEL(fks_simulate_linked_traced, THROUGHPUT, simulate_particles, F_TRACED, TRACED, THROUGHPUT, LINKED)
FKS_KERNEL(fks_simulate_se2_traced, THROUGHPUT, simulate_particles, F_TRACED, TRACED, THROUGHPUT, SE2)
FKS_KERNEL(fks_simulate_se3_traced, THROUGHPUT, simulate_particles, F_TRACED, TRACED, THROUGHPUT, SE3)

/* lean LDS blocks (LdsLayout.lean: the round skip-proof cache in the wave's scratch), chosen by
 * fks_set_robot for linked robots whose LDS block limits the resident waves (14-dof cfg5) */
FKS_KERNEL(fks_simulate_linked_lean, THROUGHPUT, simulate_particles, F_LEAN, PLAIN, THROUGHPUT, LINKED_LEAN)
FKS_KERNEL(fks_simulate_linked_lean_indiv, THROUGHPUT, simulate_particles, F_INDIVIDUAL | F_LEAN, INDIVIDUAL, THROUGHPUT, LINKED_LEAN)
FKS_KERNEL(fks_simulate_linked_lean_traced, THROUGHPUT, simulate_particles, F_TRACED | F_LEAN, TRACED, THROUGHPUT, LINKED_LEAN)

/* waypoint paths (fks_forward_simulate_path): PATH instantiations at the throughput budget ... */
FKS_KERNEL(fks_simulate_linked_path, THROUGHPUT, simulate_particles, F_PATH, PATH, THROUGHPUT, LINKED)
FKS_KERNEL(fks_simulate_linked_lean_path, THROUGHPUT, simulate_particles, F_LEAN | F_PATH, PATH, THROUGHPUT, LINKED_LEAN)
FKS_KERNEL(fks_simulate_se2_path, THROUGHPUT, simulate_particles, F_PATH, PATH, THROUGHPUT, SE2)
FKS_KERNEL(fks_simulate_se3_path, THROUGHPUT, simulate_particles, F_PATH, PATH, THROUGHPUT, SE3)
/* ... and at the small-batch budget, for paths whose batch fits its resident waves: the wave
 * carries its particle through every leg (SimArgs.path_carry) */
FKS_KERNEL(fks_simulate_linked_path_small, SMALL, simulate_particles, F_PATH, PATH, SMALL, LINKED)
FKS_KERNEL(fks_simulate_se2_path_small, SMALL, simulate_particles, F_PATH, PATH, SMALL, SE2)
FKS_KERNEL(fks_simulate_se3_path_small, SMALL, simulate_particles, F_PATH, PATH, SMALL, SE3)

/* job batches (fks_forward_simulate_jobs): JOBS instantiations at the throughput budget ... */
FKS_KERNEL(fks_simulate_linked_jobs, THROUGHPUT, simulate_particles, F_JOBS, JOBS, THROUGHPUT, LINKED)
FKS_KERNEL(fks_simulate_linked_lean_jobs, THROUGHPUT, simulate_particles, F_LEAN | F_JOBS, JOBS, THROUGHPUT, LINKED_LEAN)
FKS_KERNEL(fks_simulate_se2_jobs, THROUGHPUT, simulate_particles, F_JOBS, JOBS, THROUGHPUT, SE2)
FKS_KERNEL(fks_simulate_se3_jobs, THROUGHPUT, simulate_particles, F_JOBS, JOBS, THROUGHPUT, SE3)
/* ... and at the small-batch budget, for batches whose jobs together fit its resident waves */
FKS_KERNEL(fks_simulate_linked_jobs_small, SMALL, simulate_particles, F_JOBS, JOBS, SMALL, LINKED)
FKS_KERNEL(fks_simulate_se2_jobs_small, SMALL, simulate_particles, F_JOBS, JOBS, SMALL, SE2)
FKS_KERNEL(fks_simulate_se3_jobs_small, SMALL, simulate_particles, F_JOBS, JOBS, SMALL, SE3)

/* path-job batches (fks_forward_simulate_path_jobs): PATH && JOBS instantiations at the throughput
 * budget ... */
FKS_KERNEL(fks_simulate_linked_path_jobs, THROUGHPUT, simulate_particles, F_PATH | F_JOBS, PATH_JOBS, THROUGHPUT, LINKED)
FKS_KERNEL(fks_simulate_linked_lean_path_jobs, THROUGHPUT, simulate_particles, F_LEAN | F_PATH | F_JOBS, PATH_JOBS, THROUGHPUT, LINKED_LEAN)
FKS_KERNEL(fks_simulate_se2_path_jobs, THROUGHPUT, simulate_particles, F_PATH | F_JOBS, PATH_JOBS, THROUGHPUT, SE2)
FKS_KERNEL(fks_simulate_se3_path_jobs, THROUGHPUT, simulate_particles, F_PATH | F_JOBS, PATH_JOBS, THROUGHPUT, SE3)
/* ... and at the small-batch budget, for batches whose jobs together fit its resident waves: a
 * wave carries its particle through its own job's legs */
FKS_KERNEL(fks_simulate_linked_path_jobs_small, SMALL, simulate_particles, F_PATH | F_JOBS, PATH_JOBS, SMALL, LINKED)
FKS_KERNEL(fks_simulate_se2_path_jobs_small, SMALL, simulate_particles, F_PATH | F_JOBS, PATH_JOBS, SMALL, SE2)
FKS_KERNEL(fks_simulate_se3_path_jobs_small, SMALL, simulate_particles, F_PATH | F_JOBS, PATH_JOBS, SMALL, SE3)

/* the batched CheckConfigCollision (fks_check_config_collision) */
FKS_KERNEL(fks_check_configs_linked, THROUGHPUT, check_configs, F_NONE, CHECK, THROUGHPUT, LINKED)
FKS_KERNEL(fks_check_configs_se2, THROUGHPUT, check_configs, F_NONE, CHECK, THROUGHPUT, SE2)
FKS_KERNEL(fks_check_configs_se3, THROUGHPUT, check_configs, F_NONE, CHECK, THROUGHPUT, SE3)

/* FK, world points and the clean control input of a batch (fks_kinematics) */
FKS_KERNEL(fks_kinematics_linked, THROUGHPUT, kinematics, F_NONE, KINEMATICS, THROUGHPUT, LINKED)
FKS_KERNEL(fks_kinematics_se2, THROUGHPUT, kinematics, F_NONE, KINEMATICS, THROUGHPUT, SE2)
FKS_KERNEL(fks_kinematics_se3, THROUGHPUT, kinematics, F_NONE, KINEMATICS, THROUGHPUT, SE3)

/* policy roll-outs (fks_forward_simulate_policy): POLICY instantiations of the path kernels at the
 * throughput budget ... */
FKS_POLICY_KERNEL(fks_simulate_linked_policy, THROUGHPUT, simulate_particles, F_PATH | F_POLICY, POLICY, THROUGHPUT, LINKED)
FKS_POLICY_KERNEL(fks_simulate_linked_lean_policy, THROUGHPUT,
    simulate_particles, F_LEAN | F_PATH | F_POLICY, POLICY, THROUGHPUT, LINKED_LEAN)
FKS_POLICY_KERNEL(fks_simulate_se2_policy, THROUGHPUT, simulate_particles, F_PATH | F_POLICY, POLICY, THROUGHPUT, SE2)
FKS_POLICY_KERNEL(fks_simulate_se3_policy, THROUGHPUT, simulate_particles, F_PATH | F_POLICY, POLICY, THROUGHPUT, SE3)
/* ... and at the small-batch budget, for roll-outs whose batch fits its resident waves: the wave
 * carries its particle through every leg until it stops */
FKS_POLICY_KERNEL(fks_simulate_linked_policy_small, SMALL, simulate_particles, F_PATH | F_POLICY, POLICY, SMALL, LINKED)
FKS_POLICY_KERNEL(fks_simulate_se2_policy_small, SMALL, simulate_particles, F_PATH | F_POLICY, POLICY, SMALL, SE2)
FKS_POLICY_KERNEL(fks_simulate_se3_policy_small, SMALL, simulate_particles, F_PATH | F_POLICY, POLICY, SMALL, SE3)

#undef FKS_KERNEL
#undef FKS_POLICY_KERNEL
