/*
 * fks_launch.h — how a kernel is launched: the LDS layout, workgroup size and persistent grid of
 * a robot (fks_set_robot), which kernel a call runs and which shaped module it builds first, and
 * the grid of a launch.
 *
 * As fks_batch.h: nothing here calls the HIP runtime or reads an fks_context.  The inputs come in
 * small structs, the answers are values; what only the runtime knows (how many blocks of a kernel
 * a CU holds) is asked through Queries, which fks_capi.cpp answers with the occupancy calls and
 * tests/cpp/launch_plan_test.cpp with a table.
 */
#ifndef FKS_LAUNCH_H
#define FKS_LAUNCH_H

#include <hip/hip_vector_types.h> /* the vector types SimArgs names */
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "fks_batch.h"
#include "fks_capi.h"
#include "fks_device.h"

namespace fks_launch {

/* ---- a generic kernel's identity (FKS.cpp:4-71 factories) ----
 * Form: what the kernel does (the batched forms in the order of fks_batch::Form).  Budget:
 * throughput, or the low-occupancy instantiation for batches that fit its resident waves.
 * Family: a linked robot's lean LDS block has kernels of its own where the list has them. */
enum Form { PLAIN = 0, INDIVIDUAL, TRACED, COOPERATIVE, CHECK, KINEMATICS, PATH, JOBS, PATH_JOBS, POLICY, FORM_COUNT };
static_assert(JOBS == PATH + fks_batch::JOBS && PATH_JOBS == PATH + fks_batch::PATH_JOBS, "batched forms in Form order");
enum Budget { THROUGHPUT = 0, SMALL, BUDGET_COUNT };
enum Family { LINKED = 0, LINKED_LEAN, SE2, SE3, FAMILY_COUNT };
struct KernelId {
    Form form;
    Budget budget;
    Family family;
};
Family family_of(int32_t robot_type, bool lean);

/* the rows of fks_kernel_list.h, in its order */
constexpr int kKernelRows = 52;
/* the row of an identity, or -1: a lean robot runs the linked kernel where the list has no lean row */
int kernel_row(const KernelId& id);
const char* kernel_symbol(int row);

/* ---- the layout of a robot ---- */
constexpr size_t kCuLdsBytes = 160 * 1024;
/* the cooperative kernel's smallest workgroup (two waves) */
constexpr int kCoopMinThreads = 128;

struct RobotShape {
    int32_t type, L, J, D, W, G, P, nrounds;
};
/* what the runtime knows of a kernel; a failed query answers 0 */
struct Queries {
    /* resident blocks per CU of the kernel at `threads` per block and `lds_bytes` of dynamic LDS */
    virtual int resident_blocks(const KernelId& id, uint32_t threads, size_t lds_bytes) const = 0;
    /* the kernel's launch bound */
    virtual int max_threads(const KernelId& id) const = 0;

protected:
    ~Queries() = default;
};
struct LayoutInputs {
    RobotShape robot;
    int32_t cus;             /* compute units of the device */
    uint64_t free_hbm_bytes; /* with the current workspace, which the new one replaces */
};
struct Layout {
    bool fk_pair = false; /* paired FK of free microsteps */
    bool lean = false;    /* lean LDS block + lean kernels */
    uint32_t waves_per_cu = 0;            /* resident waves per CU (LDS and registers) */
    uint32_t standard_resident_waves = 0; /* resident waves of the non-lean layout */
    uint32_t waves_per_group = fksd::kWavesPerGroup;
    size_t lds_bytes = 0;
    uint32_t grid_groups = 0, grid_waves = 0; /* the persistent grid */
    uint64_t scratch_per_wave = 0, scratch_words = 0; /* doubles: a wave's workspace, the grid's */
    uint32_t small_grid_waves = 0; /* resident waves of the small-batch kernel (0: none for this layout) */
    uint32_t coop_particles = 0;   /* resident workgroups (particles) of the cooperative kernel (0: none) */
    uint32_t coop_waves = 0;       /* its waves per workgroup */
    size_t coop_lds_bytes = 0;
};
/* Launch geometry of a robot: the LDS layout (with the paired FK's second set of joint motion
 * matrices for linked chains of <= 32 joints when the occupancy it leaves equals the plain
 * layout's), workgroup size, resident workgroups per CU and the per-wave workspace.  FKS_OK, or
 * FKS_ERR_UNSUPPORTED with its text in *why (*out is then untouched). */
fks_status plan_layout(const LayoutInputs& in, const Queries& q, Layout* out, std::string* why);

/* ---- the kernel of a call ---- */
struct Settings {
    int32_t robot_type = FKS_ROBOT_LINKED;
    bool small_batch = true, cooperative = false, individual_jacobians = false;
    int32_t specialize = 1;     /* fks_specialization_mode */
    bool bspec_enabled = false; /* fks_set_batched_specialization */
    bool lean = false;          /* Layout.lean */
    uint32_t coop_particles = 0, grid_waves = 0; /* of the layout */
};
/* what a shaped module has */
struct ModuleState {
    bool fn = false, small_fn = false, check_fn = false;
    bool pending = false; /* robot set, the module not built yet */
};
enum RequestKind { REQUEST_PLAIN = 0, REQUEST_TRACED, REQUEST_BATCH, REQUEST_CHECK };
struct Request {
    RequestKind kind = REQUEST_PLAIN;
    fks_batch::Form form = fks_batch::PATH; /* of a batch ... */
    bool policy = false;                    /* ... a policy roll-out ... */
    uint64_t legs = 0;                      /* ... and its legs (Batch.legs) */
    uint64_t n = 0;                         /* particles (configurations of a check) */
    bool small = false;                     /* SegmentPlan.small */
    uint32_t nseg = 1;                      /* SegmentPlan.nseg */
};
enum Module { MODULE_NONE = 0, MODULE_PLAIN, MODULE_BATCHED };
enum ModuleFunction { FUNCTION_NONE = 0, FUNCTION_THROUGHPUT, FUNCTION_SMALL, FUNCTION_CHECK };
/* The pending module this launch builds first: the one whose throughput kernel it would run
 * (never for a small batch: robots only ever simulated in small batches cost no compile; never
 * for a policy roll-out or a batch of more than FKS_MAX_PATH_JOB_LEGS legs), and the plain one
 * for a check of more configurations than the grid has waves. */
Module module_to_build(const Settings& s, const ModuleState& plain, const ModuleState& batched, const Request& rq);
struct Choice {
    int32_t kind = FKS_KERNEL_NONE;  /* fks_launch_info: last_kernel (a check: last_check_kernel) */
    KernelId generic{};              /* the library's kernel of the request ... */
    Module module = MODULE_NONE;     /* ... or, when not MODULE_NONE, the module ... */
    ModuleFunction function = FUNCTION_NONE; /* ... and its function that runs instead */
    bool cooperative = false;        /* the cooperative geometry: one workgroup per particle */
};
/* ... and what then runs, with the modules as they are after that build */
Choice choose_kernel(const Settings& s, const ModuleState& plain, const ModuleState& batched, const Request& rq);

/* ---- the grid of a launch ---- */
struct Geometry {
    uint32_t blocks, threads;
    size_t lds_bytes;
};
/* workgroups of a launch over n particles, one per wave: what n needs, at most the resident
 * groups, at least one (a simulation of no particle still launches) */
uint32_t groups_launched(uint64_t n, uint32_t waves_per_group, uint32_t resident_groups);
Geometry launch_geometry(const Layout& l, uint64_t n, bool cooperative = false);

/* ---- the register gates of a shaped module ----
 * the throughput kernel's: the persistent grid is sized for the generic kernel's occupancy, so a
 * specialised kernel is used only if it needs no more registers.  512 VGPRs per SIMD lane,
 * allocated in granules of 8; waves_per_eu = 0: the generic kernel's own count */
int throughput_register_budget(int waves_per_eu, int generic_registers);
/* the small-batch kernel's: what two waves per SIMD leave */
constexpr int kSmallRegisterBound = 256;

}  // namespace fks_launch

#endif
