/*
 * fks_capi.cpp — host implementation of the C-ABI in include/fks_capi.h.
 *
 * A context mirrors one SimpleParticleContactSimulator (SPCS:371-1999): it owns
 * device copies of the SDF and the surface-normal grid (copied once, as the
 * reference copies them at construction SPCS:420), the flattened robot, the
 * solver parameters (SPCS:345-369) and the counter-based RNG stream state.
 * fks_forward_simulate replaces the OpenMP particle loop of
 * ForwardSimulateRobots (SPCS:788-804) with one launch of the persistent
 * simulation kernel.  No exceptions cross the ABI.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "fks_capi.h"
#include "fks_batch.h"
#include "fks_buffers.h"
#include "fks_env_internal.h"
#include "fks_launch.h"
#include "fks_robot.h"
#include "fks_specialize.h"
#include "fks_device.h"
#include "fks_portable_math.h"

/* the kernels that take a SimArgs: fks_kernel_list.h's rows */
#define FKS_KERNEL(symbol, ...) extern "C" __global__ void symbol(const fksd::SimArgs* args);
#define FKS_POLICY_KERNEL(symbol, ...) extern "C" __global__ void symbol(const fksd::SimArgs* args, const fksd::PolicyArgs* pol);
#include "fks_kernel_list.h"
extern "C" __global__ void fks_cluster_linked(const fksd::ClusterArgs args);
extern "C" __global__ void fks_cluster_se2(const fksd::ClusterArgs args);
extern "C" __global__ void fks_cluster_se3(const fksd::ClusterArgs args);
extern "C" __global__ void fks_summary_linked(const fksd::SummaryArgs args);
extern "C" __global__ void fks_summary_se2(const fksd::SummaryArgs args);
extern "C" __global__ void fks_summary_se3(const fksd::SummaryArgs args);
extern "C" __global__ void fks_state_select_linked(const fksd::SelectArgs args);
extern "C" __global__ void fks_state_select_se2(const fksd::SelectArgs args);
extern "C" __global__ void fks_state_select_se3(const fksd::SelectArgs args);
extern "C" __global__ void fks_state_draw(const fksd::SelectArgs args);
extern "C" __global__ void fks_math_probe(const double* a, const double* b, double* out, uint64_t n);

namespace {

using fks_launch::family_of;
using fks_launch::KernelId;

/* the list's kernels by row, each signature in an array of its own (a policy roll-out's kernels
 * take the call's PolicyArgs second); the function of an identity (fks_launch::kernel_row), null
 * where the library has none of that signature */
typedef void (*sim_kernel_t)(const fksd::SimArgs*);
typedef void (*policy_kernel_t)(const fksd::SimArgs*, const fksd::PolicyArgs*);
const sim_kernel_t kSimKernels[] = {
#define FKS_KERNEL(symbol, ...) symbol,
#define FKS_POLICY_KERNEL(symbol, ...) nullptr,
#include "fks_kernel_list.h"
};
const policy_kernel_t kPolicyKernels[] = {
#define FKS_KERNEL(symbol, ...) nullptr,
#define FKS_POLICY_KERNEL(symbol, ...) symbol,
#include "fks_kernel_list.h"
};
static_assert(sizeof(kSimKernels) / sizeof(kSimKernels[0]) == fks_launch::kKernelRows, "one function per row");
sim_kernel_t sim_kernel_of(const KernelId& id) {
    const int row = fks_launch::kernel_row(id);
    return row < 0 ? nullptr : kSimKernels[row];
}
policy_kernel_t policy_kernel_of(const KernelId& id) {
    const int row = fks_launch::kernel_row(id);
    return row < 0 ? nullptr : kPolicyKernels[row];
}
/* ... as the runtime's attribute and occupancy queries take it */
const void* kernel_of(const KernelId& id) {
    const sim_kernel_t k = sim_kernel_of(id);
    return k ? reinterpret_cast<const void*>(k) : reinterpret_cast<const void*>(policy_kernel_of(id));
}
/* the clustering and summary kernels by family (they have no lean form) */
void (*const kClusterKernels[fks_launch::FAMILY_COUNT])(const fksd::ClusterArgs) = {fks_cluster_linked, fks_cluster_linked, fks_cluster_se2,
                                                                                   fks_cluster_se3};
void (*const kSummaryKernels[fks_launch::FAMILY_COUNT])(const fksd::SummaryArgs) = {fks_summary_linked, fks_summary_linked, fks_summary_se2,
                                                                                   fks_summary_se3};

using fks_batch::splitmix64;
using fks_buf::DeviceBuffer;
using fks_buf::MirroredBuffer;

using fksd::GridDev;
/* a segment averaging this many resolver iterations per controller step is
 * contact-heavy: its wave keeps the particle (the cfg3 batch averages 0.65) ... */
constexpr uint32_t kHeavyResolverPerStep = 2;
/* ... if it also has at least this many times the batch's mean resolver iterations per
 * segment so far: a batch where most segments resolve contacts (cfg5) carries only its
 * outliers */
constexpr uint32_t kHeavyRelative = 3;
using fksd::JointDev;
using fksd::RobotDev;

inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

void inverse34(const double* T, double* I) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) I[4 * i + j] = T[4 * j + i];
    for (int i = 0; i < 3; ++i) I[4 * i + 3] = -dot3(I[4 * i + 0], I[4 * i + 1], I[4 * i + 2], T[3], T[7], T[11]);
}

GridDev make_grid(const fks_grid_geometry& g) {
    GridDev d;
    std::memcpy(d.org, g.origin, sizeof(d.org));
    inverse34(d.org, d.inv);
    d.res = g.resolution;
    d.inv_res = 1.0 / g.resolution;
    for (int a = 0; a < 3; ++a) d.n[a] = g.num_cells[a];
    for (int w = 0; w < 3; ++w) d.inv_res_span[w] = 1.0 / (g.resolution * (double)w);
    for (int a = 0; a < 3; ++a) d.nb[a] = (uint32_t)((g.num_cells[a] + 3) >> fksd::kBrickShift);
    d.nb_pad = 0;
    return d;
}


uint32_t forward_steps(double time, double frequency) {
    const double raw = time * frequency;
    if (!(raw < 4294967295.0)) return 0xffffffffu;
    const uint32_t steps = (raw > 0.0) ? (uint32_t)raw : 0u;
    return steps > 1u ? steps : 1u;
}

/* `count` elements of `src` (host or device memory) in a block of `b`'s own */
template <typename T>
hipError_t upload(DeviceBuffer<T>& b, const T* src, size_t count, hipMemcpyKind kind = hipMemcpyHostToDevice) {
    const hipError_t e = b.reserve(count);
    if (e != hipSuccess) return e;
    return hipMemcpy(b.get(), src, count * sizeof(T), kind);
}
/* a host table in a block of `b`'s own; an empty table takes none (b stays empty, its pointer null) */
template <typename T>
hipError_t upload(DeviceBuffer<T>& b, const std::vector<T>& table) {
    return table.empty() ? hipSuccess : upload(b, table.data(), table.size());
}

bool valid_grid(const fks_grid_geometry& g) {
    if (!(g.resolution > 0.0) || !std::isfinite(g.resolution)) return false;
    for (int a = 0; a < 3; ++a)
        if (g.num_cells[a] < 2 || g.num_cells[a] > 65535) return false;
    const double cells = (double)g.num_cells[0] * (double)g.num_cells[1] * (double)g.num_cells[2];
    /* the kernels address cells of the 4x4x4-brick layout with 32-bit indices */
    const double padded = (double)((g.num_cells[0] + 3) & ~3ll) * (double)((g.num_cells[1] + 3) & ~3ll) *
                          (double)((g.num_cells[2] + 3) & ~3ll);
    return cells < 4294967295.0 && padded < 4294967295.0;
}

bool same_geometry(const fks_grid_geometry& a, const fks_grid_geometry& b) {
    return std::memcmp(a.origin, b.origin, sizeof(a.origin)) == 0 && a.resolution == b.resolution &&
           a.num_cells[0] == b.num_cells[0] && a.num_cells[1] == b.num_cells[1] && a.num_cells[2] == b.num_cells[2];
}

}  // namespace

/* One robot shape's module of specialised kernels (fks_specialize.cpp), loaded on the context's
 * device: the plain module (fks_set_specialization) and the batched one of the same shape
 * (fks_set_batched_specialization) are two of these */
struct ShapedModule {
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;       /* the throughput kernel */
    hipFunction_t small_fn = nullptr; /* the small-batch kernel (non-lean shapes) */
    hipFunction_t check_fn = nullptr; /* fks_check_configs_shaped (the plain module only) */
    std::string shape;
    double seconds = 0.0;
    int32_t from_cache = 0;
    uint64_t launches = 0;
    bool failed = false;  /* the current robot's build failed (its calls run the generic kernels) */
    std::string message;  /* why (fks_specialization_info.message) */
    bool pending = false; /* robot set, the module not built yet (built at the first launch that runs it) */
};
/* what tells the two modules apart */
struct ShapedKind {
    bool batched;         /* Shape.batched */
    const char* fn;
    const char* small_fn;
    const char* check_fn; /* null: none */
    const char* noun;     /* of the register refusal */
};
static const ShapedKind kPlainModule = {false, "fks_simulate_shaped", "fks_simulate_shaped_small", "fks_check_configs_shaped", "kernel"};
static const ShapedKind kBatchedModule = {true, "fks_simulate_shaped_pj", "fks_simulate_shaped_pj_small", nullptr, "batch kernel"};

/* the current robot's tables in HBM, one block each (RobotDev points into them): the arrays of
 * the description and those fks_robot::flatten derives from it */
struct RobotBuffers {
    DeviceBuffer<JointDev> joints;
    DeviceBuffer<int32_t> geom_link;
    DeviceBuffer<uint32_t> geom_off;
    DeviceBuffer<double> points;
    DeviceBuffer<uint16_t> point_geom, point_link;
    DeviceBuffer<int32_t> dof_joint;
    DeviceBuffer<uint64_t> link_dof_mask;
    DeviceBuffer<int32_t> pairs;
    DeviceBuffer<uint64_t> allowed_mask;
    DeviceBuffer<double> geom_box, geom_mass;
    DeviceBuffer<fks_dof_controller> ctrl;
    DeviceBuffer<double> weights;
    DeviceBuffer<fksd::RoundDev> rounds;
    DeviceBuffer<double> dof_lever, dof_lever_box;
    /* sampled actuators: each sampled dof's two tables, and the SampledDev array that names them */
    struct SampledTables {
        DeviceBuffer<double> bounds, samples;
    };
    std::vector<SampledTables> sampled_tables;
    DeviceBuffer<fksd::SampledDev> sampled;
};

struct fks_context {
    int device = 0;
    std::string last_error;
    int32_t debug_level = 0;
    fks_solver_params params;
    double frequency = 1.0;
    uint64_t seed = 0;
    uint64_t call_index = 0;
    /* environment */
    DeviceBuffer<float> d_sdf;     /* bricked (fks_device.h brick_cell) */
    DeviceBuffer<uint32_t> d_noff; /* VoxelGrid-order CSR offsets, only until they are bricked */
    DeviceBuffer<uint2> d_nrange;  /* bricked [begin, end) per normal-grid cell */
    DeviceBuffer<double> d_nent;
    GridDev sdf_g, nrm_g, env_g;
    float oob = 0.0f;
    int32_t has_normals = 0;
    int32_t skip_enabled = 0;
    double skip_lplus = 0.0, skip_cmax = 0.0;
    /* robot */
    bool has_robot = false;
    RobotDev R;
    RobotBuffers robot;
    /* launch resources */
    DeviceBuffer<double> d_scratch; /* the persistent grid's per-wave workspaces */
    fks_launch::Layout lay;         /* the current robot's layout (fks_set_robot) */
    MirroredBuffer<unsigned long long> counters; /* kNumCounters + queue + phase cycles, and their pinned copy */
    uint64_t phase_last[FKS_NUM_PHASES] = {};
    uint64_t phase_total[FKS_NUM_PHASES] = {};
    MirroredBuffer<fksd::SimArgs> args; /* kernel arguments, read through a pointer, staged in pinned memory */
    DeviceBuffer<uint32_t> d_policy_choice; /* fks_forward_simulate_policy's host entry: the selection's staging */
    DeviceBuffer<double> d_policy_distance;
    DeviceBuffer<uint32_t> d_policy_legs;
    DeviceBuffer<double> d_policy_in; /* and its inputs' own: the starts with the table behind them */
    /* fks_cluster_configs_device: the staged offsets (pinned, then in HBM) and the HBM link workspace ... */
    MirroredBuffer<uint64_t> cluster_off;
    DeviceBuffer<double> d_cluster_work;
    /* ... and the host entry's staging: the configurations, the matrices, the labels and the counts */
    DeviceBuffer<double> d_cluster_in;
    DeviceBuffer<double> d_cluster_mat;
    DeviceBuffer<uint32_t> d_cluster_labels;
    DeviceBuffer<uint32_t> d_cluster_counts;
    /* fks_summarize_clusters_device: the staged offsets and the HBM workspace of the members' terms ... */
    MirroredBuffer<uint64_t> summary_off;
    DeviceBuffer<double> d_summary_work;
    /* ... and the host entry's staging: the doubles (configurations, targets, then the outputs) and the words
     * (labels, then the outputs) */
    DeviceBuffer<double> d_summary_f64;
    DeviceBuffer<uint32_t> d_summary_u32;
    /* fks_select_states_device: the search's partial results, one per (query, chunk) ... */
    DeviceBuffer<fksd::SelectPartial> d_select_partials;
    int32_t compute_units = 0; /* of the device, read at the first selection */
    /* ... and the host entry's staging: every input and output array end to end, each on an 8-byte boundary, and
     * the host copy of the inputs that goes up in one piece */
    DeviceBuffer<double> d_select_stage;
    std::vector<double> select_stage;
    MirroredBuffer<fksd::SimArgs> path_args; /* a batch's records (fks_batch::build_records): one per (job, leg) of
                                                its normal form (a path's legs, a job batch's jobs), then job_first
                                                and leg_first (SimArgs.job_first) */
    std::vector<unsigned char> jobs_stage;    /* fks_forward_simulate_jobs / _path_jobs: the jobs' inputs, then outputs, end to end */
    bool pending = false;
    int pending_kind = 0; /* 0 = forward simulation, 1 = batched config check, 2 = clustering (nothing to fold) */
    hipStream_t pending_stream = nullptr;
    fks_call_counters check_last;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::chrono::steady_clock::time_point call_start;
    fks_buf::ParticleStaging stage; /* host-API staging */
    DeviceBuffer<double> d_pid;     /* fks_forward_simulate_mutable controller state */
    /* controller-step segments: resting particle state between segments */
    uint32_t segment_steps = 0; /* 0 = automatic (kDefaultSegmentSteps) */
    uint32_t heavy_per_step = kHeavyResolverPerStep; /* fks_set_segment_policy */
    uint32_t heavy_priority = 2; /* round 6: cfg5 -2 %, cfg3 / cfg4 equal (profiles/r06prio_*.json) */
    uint32_t heavy_relative = kHeavyRelative; /* fks_set_segment_heavy_relative */
    int32_t individual_jacobians = 0; /* fks_set_individual_jacobians (SPCS:420-423) */
    int32_t small_batch = 1;          /* fks_set_small_batch_kernel */
    int32_t cooperative = 0;          /* fks_set_cooperative_waves (opt-in: DESIGN.md §5.4) */
    int32_t last_kernel = FKS_KERNEL_NONE;       /* the simulation kernel of the last call */
    int32_t last_check_kernel = FKS_KERNEL_NONE; /* the configuration-check kernel of the last check */
    DeviceBuffer<double> d_seg_state;
    DeviceBuffer<uint32_t> d_seg_done;
    fks_statistics stats;
    fks_call_counters last;
    fks_call_counters total;
    /* robot-shape specialisation (fks_set_specialization, fks_specialize.cpp) */
    int32_t specialize = 1;
    ShapedModule spec; /* fks_simulate_shaped[_small] and fks_check_configs_shaped of the current robot's shape */
    /* the batched module of the same shape (fks_set_batched_specialization): the kernels of
     * path, job and path-job batches, built at the first batch that runs its throughput kernel */
    int32_t bspec_enabled = 0; /* opt-in: fks_set_batched_specialization / fks_prepare_batched_specialization */
    ShapedModule bspec;        /* fks_simulate_shaped_pj[_small] */
};

static fks_status fail(fks_context* ctx, fks_status st, const std::string& msg) {
    if (ctx) ctx->last_error = msg;
    return st;
}
static fks_status hip_fail(fks_context* ctx, hipError_t e, const char* where) {
    return fail(ctx, FKS_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(ctx, expr)                                       \
    do {                                                         \
        hipError_t _e = (expr);                                  \
        if (_e != hipSuccess) return hip_fail((ctx), _e, #expr); \
    } while (0)

static void shaped_release(fks_context* ctx, ShapedModule* m);

static void free_robot(fks_context* ctx) {
    shaped_release(ctx, &ctx->spec); /* a specialised kernel belongs to one robot shape */
    shaped_release(ctx, &ctx->bspec);
    ctx->bspec.pending = false;
    ctx->robot = RobotBuffers();
    ctx->d_scratch.reset();
    ctx->has_robot = false;
}

/* unloads a module and clears its report; `pending` is the caller's to set */
static void shaped_release(fks_context* ctx, ShapedModule* m) {
    if (m->module) {
        (void)hipSetDevice(ctx->device);
        (void)hipModuleUnload(m->module);
    }
    const bool pending = m->pending;
    *m = ShapedModule();
    m->pending = pending;
}

/* what the specialised builds of the current robot fix at compile time */
static fks_spec::Shape spec_shape_of(const fks_context* ctx) {
    fks_spec::Shape sh;
    sh.type = ctx->R.type;
    sh.L = ctx->R.L;
    sh.J = ctx->R.J;
    sh.D = ctx->R.D;
    sh.W = ctx->R.W;
    sh.G = ctx->R.G;
    sh.P = ctx->R.P;
    sh.pair = ctx->lay.fk_pair ? 1 : 0;
    sh.lean = ctx->lay.lean ? 1 : 0;
    sh.no_proofs = ctx->specialize == FKS_SPECIALIZE_NO_PROOFS ? 1 : 0;
    /* the waves a SIMD holds at this layout (4 SIMDs per CU): when the LDS block keeps fewer
     * resident than the register budget allows (cfg5's lean blocks: 16 per CU), the
     * specialised kernel is compiled for that many and may use their registers */
    const int per_simd = (int)((ctx->lay.waves_per_cu + 3) / 4);
    if (per_simd >= 1 && per_simd < fksd::kThroughputWavesPerEU) sh.waves_per_eu = per_simd;
    /* FKS_SPEC_WAVES_PER_EU=n (tuning and A/B runs): compile for n waves per SIMD instead
     * (n >= the layout's waves; 0 = the library's budget) */
    if (const char* e = std::getenv("FKS_SPEC_WAVES_PER_EU")) {
        const int n = std::atoi(e);
        if (n == 0 || n == fksd::kThroughputWavesPerEU) sh.waves_per_eu = 0;
        else if (n >= per_simd && n <= 8) sh.waves_per_eu = n;
    }
    return sh;
}

/* the code object of `sh` (a cache or a compile) loaded on the context's device */
static fks_status spec_load(fks_context* ctx, const fks_spec::Shape& sh, std::shared_ptr<const fks_spec::CodeObject>* out_co,
                            hipModule_t* out_m, bool* out_compiled) {
    std::string log;
    bool compiled = false;
    std::shared_ptr<const fks_spec::CodeObject> co = fks_spec::code_object(sh, &log, &compiled);
    if (!co) return fail(ctx, FKS_ERR_UNSUPPORTED, "shape specialisation: " + log);
    hipModule_t m = nullptr;
    hipError_t e = hipModuleLoadData(&m, co->bytes.data());
    if (e != hipSuccess && !compiled) {
        /* a cached code object the runtime refuses (truncated, or from another toolchain):
         * dropped from both caches and compiled afresh, once */
        (void)hipGetLastError();
        co = fks_spec::code_object(sh, &log, &compiled, /*refresh=*/true);
        if (!co) return fail(ctx, FKS_ERR_UNSUPPORTED, "shape specialisation (after an unloadable cached code object): " + log);
        e = hipModuleLoadData(&m, co->bytes.data());
    }
    if (e != hipSuccess) return hip_fail(ctx, e, "hipModuleLoadData (shape-specialised kernel)");
    *out_co = co;
    *out_m = m;
    *out_compiled = compiled;
    return FKS_OK;
}

/* the throughput register budget of a shaped kernel, against the generic kernel it replaces */
static int spec_budget(const fks_context* ctx, const fks_spec::Shape& sh) {
    hipFuncAttributes gen{};
    const KernelId generic{fks_launch::PLAIN, fks_launch::THROUGHPUT, family_of(ctx->R.type, ctx->lay.lean)};
    if (hipFuncGetAttributes(&gen, kernel_of(generic)) != hipSuccess) gen.numRegs = 0;
    return fks_launch::throughput_register_budget(sh.waves_per_eu, gen.numRegs);
}

/* VGPRs plus AGPRs of kernel `name`, read from the code object's metadata (the runtime's
 * attribute query reports a different quantity for module kernels than for the library's own) */
static int spec_registers(const fks_spec::CodeObject& co, const char* name) {
    return fks_spec::kernel_metadata_uint(co.bytes, name, ".vgpr_count") +
           std::max(0, fks_spec::kernel_metadata_uint(co.bytes, name, ".agpr_count"));
}

/* A module of the current robot: compiled (or taken from a cache), loaded on the context's
 * device, and used only if its throughput kernel keeps the generic kernel's occupancy (the
 * persistent grid is sized for that).  The batched module (Shape.batched) applies the plain
 * module's rules to path, job and path-job batches: the same register gates */
static fks_status shaped_build(fks_context* ctx, ShapedModule* sm, const ShapedKind& kind) {
    fks_spec::Shape sh = spec_shape_of(ctx);
    sh.batched = kind.batched ? 1 : 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    sm->shape = fks_spec::shape_key(sh); /* named in the report even when the build fails */
    std::shared_ptr<const fks_spec::CodeObject> co;
    hipModule_t m = nullptr;
    hipFunction_t f = nullptr;
    bool compiled = false;
    const fks_status ld = spec_load(ctx, sh, &co, &m, &compiled);
    if (ld != FKS_OK) return ld;
    const hipError_t e = hipModuleGetFunction(&f, m, kind.fn);
    if (e != hipSuccess) {
        (void)hipModuleUnload(m);
        return hip_fail(ctx, e, ("hipModuleGetFunction(" + std::string(kind.fn) + ")").c_str());
    }
    const int shaped_vgpr = spec_registers(*co, kind.fn);
    const int budget = spec_budget(ctx, sh);
    if (shaped_vgpr <= 0 || shaped_vgpr > budget) {
        (void)hipModuleUnload(m);
        return fail(ctx, FKS_ERR_UNSUPPORTED,
                    "shape specialisation: the specialised " + std::string(kind.noun) + " needs " + std::to_string(shaped_vgpr) +
                        " VGPRs, the budget is " + std::to_string(budget));
    }
    sm->module = m;
    sm->fn = f;
    /* the configuration check of the same shape, when the module carries it */
    hipFunction_t fc = nullptr;
    if (kind.check_fn && hipModuleGetFunction(&fc, m, kind.check_fn) == hipSuccess) sm->check_fn = fc;
    /* ... and the small-batch kernel, used when it needs no more registers than two waves per
     * SIMD leave (the generic small-batch kernel's grid is the one launched) */
    hipFunction_t fs = nullptr;
    if (!ctx->lay.lean && hipModuleGetFunction(&fs, m, kind.small_fn) == hipSuccess) {
        const int v = spec_registers(*co, kind.small_fn);
        if (v > 0 && v <= fks_launch::kSmallRegisterBound) sm->small_fn = fs;
    }
    (void)hipGetLastError();
    sm->seconds = compiled ? co->compile_seconds : 0.0;
    sm->from_cache = compiled ? 0 : 1;
    return FKS_OK;
}

/* Releases the module and builds it for the current robot when the mode allows it: the plain
 * module for any specialisation mode, the batched one only for FKS_SPECIALIZE_ON.  A failure
 * leaves the generic kernels in place and is recorded (fks_specialization_info.failed / message) */
static fks_status shaped_prepare(fks_context* ctx, ShapedModule* sm, const ShapedKind& kind) {
    shaped_release(ctx, sm);
    const bool allowed = kind.batched ? ctx->specialize == FKS_SPECIALIZE_ON : ctx->specialize != 0;
    if (!allowed || !ctx->has_robot) return FKS_OK;
    const fks_status st = shaped_build(ctx, sm, kind);
    if (st != FKS_OK) {
        sm->failed = true;
        sm->message = ctx->last_error;
        /* a failed module load can leave the runtime's per-thread error set; the generic
         * launch that follows checks hipGetLastError and must not pick it up */
        (void)hipGetLastError();
    }
    return st;
}

/* the build at the first launch that runs a pending module: a failure keeps the generic kernels
 * and adds to the last error (fks_get_specialization / fks_get_last_error) without failing the call */
static void shaped_build_pending(fks_context* ctx, ShapedModule* sm, const ShapedKind& kind) {
    sm->pending = false;
    const std::string keep = ctx->last_error;
    if (shaped_prepare(ctx, sm, kind) != FKS_OK) ctx->last_error = keep + (keep.empty() ? "" : "; ") + ctx->last_error;
    (void)hipSetDevice(ctx->device);
}

/* what the kernel decision (fks_launch.h) reads of the context and of a module */
static fks_launch::Settings launch_settings(const fks_context* ctx) {
    fks_launch::Settings s;
    s.robot_type = ctx->R.type;
    s.small_batch = ctx->small_batch != 0;
    s.cooperative = ctx->cooperative != 0;
    s.individual_jacobians = ctx->individual_jacobians != 0;
    s.specialize = ctx->specialize;
    s.bspec_enabled = ctx->bspec_enabled != 0;
    s.lean = ctx->lay.lean;
    s.coop_particles = ctx->lay.coop_particles;
    s.grid_waves = ctx->lay.grid_waves;
    return s;
}
static fks_launch::ModuleState module_state(const ShapedModule& m) {
    return fks_launch::ModuleState{m.fn != nullptr, m.small_fn != nullptr, m.check_fn != nullptr, m.pending};
}

/* The kernel of a request: the pending module the decision names is built first, then the decision
 * is taken on what there is.  *module and *function: the shaped one that runs, or null */
static fks_launch::Choice decide_kernel(fks_context* ctx, const fks_launch::Request& rq, ShapedModule** module, hipFunction_t* function) {
    const fks_launch::Settings s = launch_settings(ctx);
    switch (fks_launch::module_to_build(s, module_state(ctx->spec), module_state(ctx->bspec), rq)) {
        case fks_launch::MODULE_PLAIN: shaped_build_pending(ctx, &ctx->spec, kPlainModule); break;
        case fks_launch::MODULE_BATCHED: shaped_build_pending(ctx, &ctx->bspec, kBatchedModule); break;
        case fks_launch::MODULE_NONE: break;
    }
    const fks_launch::Choice c = fks_launch::choose_kernel(s, module_state(ctx->spec), module_state(ctx->bspec), rq);
    ShapedModule* m = c.module == fks_launch::MODULE_PLAIN ? &ctx->spec : (c.module == fks_launch::MODULE_BATCHED ? &ctx->bspec : nullptr);
    *module = m;
    *function = !m ? nullptr
                   : (c.function == fks_launch::FUNCTION_SMALL ? m->small_fn
                                                               : (c.function == fks_launch::FUNCTION_CHECK ? m->check_fn : m->fn));
    return c;
}

extern "C" {

int fks_abi_version(void) { return FKS_ABI_VERSION; }

const char* fks_status_string(fks_status status) {
    switch (status) {
        case FKS_OK: return "ok";
        case FKS_ERR_INVALID_ARGUMENT: return "invalid argument";
        case FKS_ERR_HIP: return "HIP runtime error";
        case FKS_ERR_NO_ROBOT: return "no robot set";
        case FKS_ERR_OUT_OF_MEMORY: return "out of memory";
        case FKS_ERR_UNSUPPORTED: return "unsupported";
        case FKS_ERR_NO_DEVICE: return "no HIP device";
        default: return "unknown status";
    }
}

fks_status fks_default_solver_params(fks_solver_params* out) {
    if (!out) return FKS_ERR_INVALID_ARGUMENT;
    /* SimulatorSolverParameters() defaults, SPCS:357-368 */
    out->forward_simulation_time = 1.0;
    out->simulation_shortcut_distance = 0.0;
    out->environment_collision_check_tolerance = 0.001;
    out->resolve_correction_step_scaling_decay_rate = 0.5;
    out->resolve_correction_initial_step_size = 1.0;
    out->resolve_correction_min_step_scaling = 0.03125;
    out->max_resolver_iterations = 25;
    out->resolve_correction_step_scaling_decay_iterations = 5;
    out->failed_resolves_end_motion = 1;
    out->reserved = 0;
    return FKS_OK;
}

/* fks_create / fks_create_from_device_env: the environment comes either from host
 * arrays (henv) or from a device-resident GPU build (denv) */
static fks_status create_impl(const fks_environment* henv, const fks_device_env* denv, const fks_solver_params* params,
                              double simulation_controller_frequency, uint64_t prng_seed, int32_t debug_level, int32_t device,
                              fks_context** out_ctx) {
    if (!out_ctx) return FKS_ERR_INVALID_ARGUMENT;
    *out_ctx = nullptr;
    if (!params || (!henv && !denv)) return FKS_ERR_INVALID_ARGUMENT;
    if (henv) {
        if (!henv->sdf_values) return FKS_ERR_INVALID_ARGUMENT;
        if (!valid_grid(henv->sdf) || !valid_grid(henv->collision_map) || !valid_grid(henv->normals)) return FKS_ERR_INVALID_ARGUMENT;
    } else if (!valid_grid(denv->geometry) || !denv->sdf || !denv->offsets) {
        return FKS_ERR_INVALID_ARGUMENT;
    }
    if (!(simulation_controller_frequency != 0.0) || !std::isfinite(simulation_controller_frequency)) return FKS_ERR_INVALID_ARGUMENT;
    if (params->resolve_correction_step_scaling_decay_iterations == 0) return FKS_ERR_INVALID_ARGUMENT;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return FKS_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return FKS_ERR_INVALID_ARGUMENT;
    /* destroyed with whatever it owns by then on every early return */
    std::unique_ptr<fks_context, void (*)(fks_context*)> ctx(new (std::nothrow) fks_context(), fks_destroy);
    if (!ctx) return FKS_ERR_OUT_OF_MEMORY;
    ctx->device = device;
    ctx->params = *params;
    ctx->frequency = simulation_controller_frequency;
    ctx->seed = prng_seed;
    ctx->debug_level = debug_level;
    {
        const char* sp = std::getenv("FKS_SPECIALIZE");
        ctx->specialize = (sp && std::string(sp) == "0") ? 0 : 1;
    }
    std::memset(&ctx->stats, 0, sizeof(ctx->stats));
    std::memset(&ctx->last, 0, sizeof(ctx->last));
    std::memset(&ctx->total, 0, sizeof(ctx->total));
    if (hipSetDevice(device) != hipSuccess) return FKS_ERR_HIP;
    double lp = 0.0, cm = 0.0;
    bool analyzed = false;
    if (henv) {
        ctx->sdf_g = make_grid(henv->sdf);
        ctx->nrm_g = make_grid(henv->normals);
        ctx->env_g = make_grid(henv->collision_map);
        ctx->oob = henv->sdf_oob_value;
        const size_t cells = (size_t)henv->sdf.num_cells[0] * (size_t)henv->sdf.num_cells[1] * (size_t)henv->sdf.num_cells[2];
        if (upload(ctx->d_sdf, henv->sdf_values, cells) != hipSuccess) return FKS_ERR_HIP;
        analyzed = fks_robot::analyze_sdf(henv->sdf_values, henv->sdf.num_cells[0], henv->sdf.num_cells[1], henv->sdf.num_cells[2],
                                          henv->sdf.resolution, &lp, &cm);
        /* an initialized grid with no stored entries (every cell empty: a lookup in bounds finds
         * the zero normal, SPCS:219-222) has offsets and may have no entry array */
        if (henv->normal_offsets) {
            const size_t ncells =
                (size_t)henv->normals.num_cells[0] * (size_t)henv->normals.num_cells[1] * (size_t)henv->normals.num_cells[2];
            const size_t entries = henv->normal_offsets[ncells];
            if (entries > 0 && !henv->normal_entries) return FKS_ERR_INVALID_ARGUMENT;
            if (upload(ctx->d_noff, henv->normal_offsets, ncells + 1) != hipSuccess) return FKS_ERR_HIP;
            if (entries > 0 && upload(ctx->d_nent, henv->normal_entries, 6 * entries) != hipSuccess) return FKS_ERR_HIP;
            ctx->has_normals = 1;
        }
    } else {
        /* the GPU build's grids coincide (SEB.cpp builds all three on one grid); +inf out of bounds */
        ctx->sdf_g = make_grid(denv->geometry);
        ctx->nrm_g = ctx->sdf_g;
        ctx->env_g = ctx->sdf_g;
        ctx->oob = std::numeric_limits<float>::infinity();
        const size_t cells = (size_t)denv->cells;
        if (upload(ctx->d_sdf, denv->sdf, cells, hipMemcpyDeviceToDevice) != hipSuccess) return FKS_ERR_HIP;
        analyzed = fks_env::analyze_sdf_device(ctx->d_sdf.get(), denv->geometry.num_cells[0], denv->geometry.num_cells[1],
                                               denv->geometry.num_cells[2], denv->geometry.resolution, &lp, &cm);
        if (upload(ctx->d_noff, denv->offsets, cells + 1, hipMemcpyDeviceToDevice) != hipSuccess) return FKS_ERR_HIP;
        if (denv->num_entries > 0 &&
            upload(ctx->d_nent, denv->entries, 6 * (size_t)denv->num_entries, hipMemcpyDeviceToDevice) != hipSuccess)
            return FKS_ERR_HIP;
        ctx->has_normals = 1;
    }
    /* the check proof's first arm shows every reachable cell positive, which rules a collision out
     * only while the threshold -tolerance * res (thr_env) is not above zero: a negative tolerance
     * makes positive cells below it collide (SPCS:923), so such a simulator evaluates every round */
    const double thr_env = 0.0 - (params->environment_collision_check_tolerance * ctx->sdf_g.res);
    if (analyzed && thr_env <= 0.0) {
        ctx->skip_enabled = 1;
        ctx->skip_lplus = lp * (1.0 + 1e-6) + 1e-6;
        ctx->skip_cmax = cm * (1.0 + 1e-6) + 1e-6;
    }
    /* the kernels' HBM layout: the SDF and the normal ranges in 4x4x4-cell bricks (the
     * analysis above read the VoxelGrid order) */
    {
        /* the bricking allocates its output (none on a failure), which replaces its input */
        float* bricked = nullptr;
        if (fks_env::brick_sdf_device(ctx->d_sdf.get(), ctx->sdf_g.n, ctx->sdf_g.nb, &bricked) != hipSuccess) return FKS_ERR_HIP;
        ctx->d_sdf.adopt(bricked, (size_t)fksd::brick_total(ctx->sdf_g.nb));
        if (ctx->d_noff.get()) {
            uint2* ranges = nullptr;
            if (fks_env::brick_normal_ranges_device(ctx->d_noff.get(), ctx->nrm_g.n, ctx->nrm_g.nb, &ranges) != hipSuccess)
                return FKS_ERR_HIP;
            ctx->d_nrange.adopt(ranges, (size_t)fksd::brick_total(ctx->nrm_g.nb));
            ctx->d_noff.reset();
        }
    }
    if (ctx->counters.reserve(fksd::kCounterWords) != hipSuccess) return FKS_ERR_HIP;
    if (ctx->args.reserve(1) != hipSuccess) return FKS_ERR_HIP;
    if (hipEventCreate(&ctx->ev0) != hipSuccess) return FKS_ERR_HIP;
    if (hipEventCreate(&ctx->ev1) != hipSuccess) return FKS_ERR_HIP;
    (void)same_geometry;
    *out_ctx = ctx.release();
    return FKS_OK;
}

fks_status fks_create(const fks_environment* env, const fks_solver_params* params, double simulation_controller_frequency,
                      uint64_t prng_seed, int32_t debug_level, int32_t device, fks_context** out_ctx) {
    if (!env) return FKS_ERR_INVALID_ARGUMENT;
    return create_impl(env, nullptr, params, simulation_controller_frequency, prng_seed, debug_level, device, out_ctx);
}

fks_status fks_create_from_device_env(const fks_device_env* env, const fks_solver_params* params,
                                      double simulation_controller_frequency, uint64_t prng_seed, int32_t debug_level,
                                      fks_context** out_ctx) {
    if (!env) return FKS_ERR_INVALID_ARGUMENT;
    return create_impl(nullptr, env, params, simulation_controller_frequency, prng_seed, debug_level, env->device, out_ctx);
}

void fks_destroy(fks_context* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->pending && ctx->pending_stream) (void)hipStreamSynchronize(ctx->pending_stream);
    (void)hipDeviceSynchronize();
    shaped_release(ctx, &ctx->spec);
    shaped_release(ctx, &ctx->bspec);
    free_robot(ctx);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    delete ctx; /* every buffer goes with its owner, on the device selected above */
}

const char* fks_get_last_error(const fks_context* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int32_t fks_config_width(const fks_context* ctx) { return (ctx && ctx->has_robot) ? ctx->R.W : 0; }

/* the occupancy calls behind fks_launch::plan_layout's questions: a failure answers 0 */
struct RuntimeQueries final : fks_launch::Queries {
    int resident_blocks(const KernelId& id, uint32_t threads, size_t lds_bytes) const override {
        int n = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel_of(id), (int)threads, lds_bytes) == hipSuccess ? n : 0;
    }
    int max_threads(const KernelId& id) const override {
        hipFuncAttributes fa{};
        return hipFuncGetAttributes(&fa, kernel_of(id)) == hipSuccess ? fa.maxThreadsPerBlock : 0;
    }
};

/* Launch geometry of the current robot: fks_launch::plan_layout on what the device answers, and
 * the workspace it asks for.  Committed to ctx only when all of it succeeds. */
static fks_status launch_layout(fks_context* ctx, const fksd::RobotDev& R) {
    fks_launch::LayoutInputs in{};
    in.robot = fks_launch::RobotShape{R.type, R.L, R.J, R.D, R.W, R.G, R.P, R.nrounds};
    HIP_TRY(ctx, hipDeviceGetAttribute(&in.cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    in.free_hbm_bytes = free_b + ctx->d_scratch.capacity() * sizeof(double); /* the current workspace is given back below */
    fks_launch::Layout lay;
    std::string why;
    const fks_status st = fks_launch::plan_layout(in, RuntimeQueries(), &lay, &why);
    if (st != FKS_OK) return fail(ctx, st, why);
    HIP_TRY(ctx, ctx->d_scratch.reserve((size_t)lay.scratch_words)); /* frees the current workspace before it allocates a larger one */
    (void)hipGetLastError(); /* an occupancy query that failed leaves the runtime's error set */
    ctx->lay = lay;
    return FKS_OK;
}

fks_status fks_set_robot(fks_context* ctx, const fks_robot_desc* d) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!d) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "null robot");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->pending && ctx->pending_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->pending_stream));
    fks_robot::Flat flat;
    {
        std::string why;
        const fks_status st = fks_robot::flatten(d, &flat, &why);
        if (st != FKS_OK) return fail(ctx, st, why); /* the previous robot stays in place */
    }
    free_robot(ctx);
    RobotBuffers& B = ctx->robot;
    RobotDev R = flat.R;
    HIP_TRY(ctx, upload(B.joints, flat.joints));
    HIP_TRY(ctx, upload(B.geom_link, d->geometry_link, (size_t)R.G));
    HIP_TRY(ctx, upload(B.geom_off, d->geometry_point_offset, (size_t)R.G + 1));
    HIP_TRY(ctx, upload(B.points, d->points, 4 * (size_t)R.P));
    HIP_TRY(ctx, upload(B.point_geom, flat.point_geom));
    HIP_TRY(ctx, upload(B.point_link, flat.point_link));
    HIP_TRY(ctx, upload(B.dof_joint, flat.dof_joint));
    HIP_TRY(ctx, upload(B.link_dof_mask, flat.link_dof_mask));
    HIP_TRY(ctx, upload(B.pairs, flat.pairs));
    HIP_TRY(ctx, upload(B.allowed_mask, flat.allowed_mask));
    HIP_TRY(ctx, upload(B.geom_box, flat.geom_box));
    HIP_TRY(ctx, upload(B.geom_mass, flat.geom_mass));
    HIP_TRY(ctx, upload(B.ctrl, d->controllers, (size_t)R.D));
    HIP_TRY(ctx, upload(B.weights, flat.weights));
    HIP_TRY(ctx, upload(B.rounds, flat.rounds));
    HIP_TRY(ctx, upload(B.dof_lever, flat.dof_lever));
    HIP_TRY(ctx, upload(B.dof_lever_box, flat.dof_lever_box));
    R.joints = B.joints.get();
    R.geom_link = B.geom_link.get();
    R.geom_off = B.geom_off.get();
    R.points = B.points.get();
    R.point_geom = B.point_geom.get();
    R.point_link = B.point_link.get();
    R.dof_joint = B.dof_joint.get();
    R.link_dof_mask = B.link_dof_mask.get();
    R.pairs = B.pairs.get();
    R.allowed_mask = B.allowed_mask.get();
    R.geom_box = B.geom_box.get();
    R.geom_mass = B.geom_mass.get();
    R.ctrl = B.ctrl.get();
    R.weights = B.weights.get();
    R.rounds = B.rounds.get();
    R.dof_lever = B.dof_lever.get();
    R.dof_lever_box = B.dof_lever_box.get();
    /* SampledUncertainVelocityActuator tables (UNC:123-281), checked by flatten */
    if (d->sampled_actuators) {
        std::vector<fksd::SampledDev> sd((size_t)R.D);
        for (int k = 0; k < R.D; ++k) {
            const fks_sampled_actuator& a = d->sampled_actuators[k];
            std::memset(&sd[k], 0, sizeof(sd[k]));
            if (a.num_bins == 0) continue;
            B.sampled_tables.emplace_back();
            RobotBuffers::SampledTables& t = B.sampled_tables.back();
            HIP_TRY(ctx, upload(t.bounds, a.bin_bounds, 2 * (size_t)a.num_bins));
            HIP_TRY(ctx, upload(t.samples, a.bin_samples, (size_t)a.num_bins * a.bin_elements));
            sd[k].nbins = a.num_bins;
            sd[k].elems = a.bin_elements;
            sd[k].bounds = t.bounds.get();
            sd[k].samples = t.samples.get();
            R.sampled_mask |= 1ull << k;
        }
        HIP_TRY(ctx, upload(B.sampled, sd));
        R.sampled = B.sampled.get();
    }
    {
        const fks_status st = launch_layout(ctx, R);
        if (st != FKS_OK) return st; /* has_robot stays false (free_robot above) */
    }
    ctx->R = R;
    ctx->has_robot = true;
    /* the new robot's shape-specialised kernel is built at the first launch that runs it
     * (simulate_device), so robots only ever simulated in small batches cost no compile */
    shaped_release(ctx, &ctx->spec);
    ctx->spec.pending = ctx->specialize != 0;
    /* ... and its batched module at the first path, job or path-job batch that runs it */
    shaped_release(ctx, &ctx->bspec);
    ctx->bspec.pending = ctx->specialize == FKS_SPECIALIZE_ON;
    return FKS_OK;
}

/* fold the counters of a finished launch into the statistics */
static fks_status settle(fks_context* ctx) {
    if (!ctx->pending) return FKS_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->pending_stream));
    ctx->pending = false;
    if (ctx->pending_kind == 2) return FKS_OK; /* a clustering call: no counters, no statistics */
    const unsigned long long* c = ctx->counters.host();
    if (ctx->pending_kind == 1) {
        /* a config check: no simulator statistics, only its own counters */
        float ms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->check_last.sdf_bytes = c[fksd::kCntSdfBytes];
        ctx->check_last.kernel_ms = (double)ms;
        ctx->check_last.call_ms =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->call_start).count();
        ctx->check_last.calls = 1;
        return FKS_OK;
    }
    ctx->stats.successful_resolves += c[fksd::kCntSuccessful];
    ctx->stats.unsuccessful_resolves += c[fksd::kCntUnsuccessful];
    ctx->stats.free_resolves += c[fksd::kCntFree];
    ctx->stats.collision_resolves += c[fksd::kCntCollision];
    ctx->stats.fallback_resolves += c[fksd::kCntFallback];
    ctx->stats.unsuccessful_env_collision_resolves += c[fksd::kCntUnsuccessfulEnv];
    ctx->stats.unsuccessful_self_collision_resolves += c[fksd::kCntUnsuccessfulSelf];
    ctx->stats.recovered_unsuccessful_resolves += c[fksd::kCntRecovered];
    ctx->last.controller_steps = c[fksd::kCntSteps];
    ctx->last.microsteps = c[fksd::kCntMicrosteps];
    ctx->last.resolver_iterations = c[fksd::kCntResolver];
    ctx->last.sdf_bytes = c[fksd::kCntSdfBytes];
    ctx->last.error_particles = c[fksd::kCntErrorParticles];
    ctx->last.least_squares_rows = c[fksd::kCntLsqRows];
    ctx->last.self_collision_checks = c[fksd::kCntSelfChecks];
    ctx->last.self_corrected_points = c[fksd::kCntSelfPoints];
    for (int k = 0; k < FKS_NUM_PHASES; ++k) {
        ctx->phase_last[k] = c[fksd::kPhaseBase + k];
        ctx->phase_total[k] += ctx->phase_last[k];
    }
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->last.kernel_ms = (double)ms;
    ctx->last.call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->call_start).count();
    ctx->last.calls = 1;
    /* a policy roll-out's particles are the (particle, leg) pairs its kernel simulated (0 otherwise) */
    ctx->last.particles += c[fksd::kCntPolicyPairs];
    ctx->total.particles += ctx->last.particles;
    ctx->total.controller_steps += ctx->last.controller_steps;
    ctx->total.microsteps += ctx->last.microsteps;
    ctx->total.resolver_iterations += ctx->last.resolver_iterations;
    ctx->total.sdf_bytes += ctx->last.sdf_bytes;
    ctx->total.error_particles += ctx->last.error_particles;
    ctx->total.least_squares_rows += ctx->last.least_squares_rows;
    ctx->total.self_collision_checks += ctx->last.self_collision_checks;
    ctx->total.self_corrected_points += ctx->last.self_corrected_points;
    ctx->total.kernel_ms += ctx->last.kernel_ms;
    ctx->total.call_ms += ctx->last.call_ms;
    ctx->total.calls += 1;
    return FKS_OK;
}

}  // extern "C"

/* device trace buffers of a traced launch (fks_forward_simulate_traced) */
struct TraceDev {
    double* inputs;
    uint32_t* micro;
    double* cfg;
    uint32_t* tags;
    uint32_t* nsteps;
    uint32_t* ncfg;
    uint32_t step_cap, cfg_cap;
};

/* the arguments every kernel that takes a SimArgs reads: the grids, the robot, the solver
 * parameters and the layout with its workspace; for the simulation and the configuration check
 * also the environment and the counters (the kinematics leaves them zero); everything else zero */
static fksd::SimArgs base_args(const fks_context* ctx, bool environment) {
    fksd::SimArgs a;
    std::memset(&a, 0, sizeof(a));
    a.sdf_g = ctx->sdf_g;
    a.nrm_g = ctx->nrm_g;
    a.env_g = ctx->env_g;
    a.R = ctx->R;
    a.S = ctx->params;
    a.scratch = ctx->d_scratch.get();
    a.scratch_per_wave = ctx->lay.scratch_per_wave;
    a.row_cap = 3u * (uint32_t)ctx->R.P;
    a.L = fksd::make_lds_layout(ctx->R.L, ctx->R.J, ctx->R.D, ctx->R.W, ctx->R.G, ctx->R.nrounds, ctx->lay.fk_pair, ctx->lay.lean);
    a.SL = fksd::make_scratch_layout(a.row_cap, ctx->R.D, ctx->R.P, ctx->R.G);
    if (!environment) return a;
    a.sdf = ctx->d_sdf.get();
    a.nrange = ctx->d_nrange.get();
    a.nent = ctx->d_nent.get();
    a.oob = ctx->oob;
    a.has_normals = ctx->has_normals;
    a.counters = ctx->counters.dev();
    a.queue = ctx->counters.dev() + fksd::kNumCounters;
    return a;
}

/* what the plan of a launch (fks_batch.h) reads of the context: its schedule settings and the
 * arguments every call on it shares */
static void plan_inputs(const fks_context* ctx, fks_batch::Inputs* in) {
    in->seed = ctx->seed;
    in->call_index = ctx->call_index;
    in->T = forward_steps(ctx->params.forward_simulation_time, std::fabs(ctx->frequency));
    in->segment_steps = ctx->segment_steps;
    in->grid_waves = ctx->lay.grid_waves;
    in->small_grid_waves = ctx->lay.small_grid_waves;
    in->small_batch = ctx->small_batch != 0;
    in->individual_jacobians = ctx->individual_jacobians != 0;
    in->lean = ctx->lay.lean;
    in->W = (uint32_t)ctx->R.W;
    in->seg_stride = 2u * (uint32_t)ctx->R.D + 4u + (uint32_t)fksd::kRoundState * (uint32_t)std::min(ctx->R.nrounds, 64);
    in->heavy_per_step = ctx->heavy_per_step;
    in->heavy_priority = ctx->heavy_priority;
    in->heavy_relative = ctx->heavy_relative;
    fksd::SimArgs& a = in->base;
    a = base_args(ctx, true);
    a.skip_enabled = ctx->skip_enabled;
    a.skip_lplus = ctx->skip_lplus;
    a.skip_cmax = ctx->skip_cmax;
    a.dt = 1.0 / ctx->frequency;
    a.thr_env = 0.0 - (ctx->params.environment_collision_check_tolerance * ctx->sdf_g.res);
    a.target_micro = ctx->env_g.res * 0.125;
    a.allowed_micro = ctx->env_g.res * 1.0;
    a.time_multiplier = 1.0 / a.dt;
    a.T = in->T;
    a.individual_jacobians = ctx->individual_jacobians;
    a.seg_stride = in->seg_stride;
}

/* One launch of a simulation kernel: a plain call (device buffers; optionally traced, or over
 * the particles' own controller state), or a batch that its entry has checked and planned. */
struct SimRequest {
    fks_job plain{};                           /* a plain call's arguments ... */
    const TraceDev* trace = nullptr;           /* fks_forward_simulate_traced */
    double* d_pid_io = nullptr;                /* fks_forward_simulate_mutable */
    const fks_batch::Batch* batch = nullptr;   /* ... or a batch in its normal form, */
    const fks_batch::Inputs* inputs = nullptr; /* with the inputs it was planned from */
    void* stream = nullptr;
    int32_t synchronize = 1;
};

static fks_job plain_call(const double* d_starts, uint64_t n, const double* d_targets, uint64_t num_targets, uint64_t first_particle_id,
                          int32_t allow_contacts, double* d_out_positions, uint8_t* d_out_collided, uint32_t* d_out_microsteps,
                          uint32_t* d_out_resolver_iterations, uint32_t* d_out_error_flags) {
    fks_job c{};
    c.starts = d_starts;
    c.n = n;
    c.targets = d_targets;
    c.num_targets = num_targets;
    c.first_particle_id = first_particle_id;
    c.allow_contacts = allow_contacts;
    c.out_positions = d_out_positions;
    c.out_collided = d_out_collided;
    c.out_microsteps = d_out_microsteps;
    c.out_resolver_iterations = d_out_resolver_iterations;
    c.out_error_flags = d_out_error_flags;
    return c;
}

/* From the zeroed counters to the queued copy of them: decides the kernel of `what` (decide_kernel),
 * launches it over `args` between the two events (a policy roll-out's kernel with `pol`) and leaves
 * the call pending or settled.  *kind: last_kernel, or last_check_kernel of a check */
static fks_status launch_request(fks_context* ctx, const fks_launch::Request& what, const fksd::SimArgs* args,
                                 const fksd::PolicyArgs* pol, hipStream_t s, int32_t synchronize, int32_t* kind) {
    const bool check = what.kind == fks_launch::REQUEST_CHECK;
    HIP_TRY(ctx, hipMemsetAsync(ctx->counters.dev(), 0, fksd::kCounterWords * sizeof(unsigned long long), s));
    ShapedModule* module = nullptr;
    hipFunction_t shaped = nullptr;
    const fks_launch::Choice l = decide_kernel(ctx, what, &module, &shaped);
    const fks_launch::Geometry g = fks_launch::launch_geometry(ctx->lay, what.n, l.cooperative);
    /* the list has a kernel of this identity, of the signature that is launched */
    const sim_kernel_t kernel = sim_kernel_of(l.generic);
    const policy_kernel_t policy = policy_kernel_of(l.generic);
    if (!shaped && !(pol ? policy != nullptr : kernel != nullptr)) return fail(ctx, FKS_ERR_UNSUPPORTED, "no kernel for this request");
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, s));
    if (!check) *kind = l.kind; /* a simulation reports its kernel also when the launch fails, a check only once it is issued */
    if (shaped) {
        void* params[] = {&args};
        HIP_TRY(ctx, hipModuleLaunchKernel(shaped, g.blocks, 1, 1, g.threads, 1, 1, (unsigned)g.lds_bytes, s, params, nullptr));
        if (!check) module->launches++;
    } else if (pol) {
        hipLaunchKernelGGL(policy, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, args, pol);
    } else {
        hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, args);
    }
    if (check) *kind = l.kind;
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->counters.host(), ctx->counters.dev(), fksd::kCounterWords * sizeof(unsigned long long),
                                hipMemcpyDeviceToHost, s));
    ctx->pending = true;
    ctx->pending_kind = check ? 1 : 0;
    ctx->pending_stream = s;
    return synchronize ? settle(ctx) : FKS_OK;
}

static fks_status simulate_device(fks_context* ctx, const SimRequest& rq) {
    const fks_batch::Batch* batch = rq.batch; /* checked by its entry (fks_batch::check_arguments, plan_batch) */
    const fks_job& call = rq.plain;
    const TraceDev* tr = rq.trace;
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    if (!batch) {
        if (call.n > 0 && (!call.starts || !call.targets || !call.out_positions))
            return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "null device buffer");
        if (call.n > 0 && call.num_targets != 1 && call.num_targets != call.n)
            return fail(ctx, FKS_ERR_INVALID_ARGUMENT, fks_batch::kTargetsOneOrN);
        if (call.n > 0xffffffffull) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "at most 2^32-1 particles per call");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(rq.stream);
    ctx->call_start = std::chrono::steady_clock::now();
    fks_batch::Inputs plain_inputs;
    if (!batch) plan_inputs(ctx, &plain_inputs);
    const fks_batch::Inputs& in = batch ? *rq.inputs : plain_inputs;
    const uint64_t n = batch ? batch->total : call.n;
    fks_batch::RecordPlan records;
    if (batch) records = fks_batch::plan_records(*batch);
    ctx->call_index += batch ? records.call_advance : 1u;
    std::memset(&ctx->last, 0, sizeof(ctx->last));
    ctx->last.particles = batch ? records.particles : n;
    if (batch && !records.launch) return FKS_OK;
    const fks_batch::SegmentPlan plan = batch ? batch->plan : fks_batch::plan_segments(in, n, 1, /*segmentable=*/!tr);
    double* seg_state = nullptr;
    uint32_t* seg_done = nullptr;
    if (plan.seg_state_words) {
        HIP_TRY(ctx, ctx->d_seg_state.reserve((size_t)plan.seg_state_words));
        seg_state = ctx->d_seg_state.get();
    }
    if (plan.seg_done_words) {
        HIP_TRY(ctx, ctx->d_seg_done.reserve((size_t)plan.seg_done_words));
        seg_done = ctx->d_seg_done.get();
        HIP_TRY(ctx, hipMemsetAsync(seg_done, 0, (size_t)plan.seg_done_words * sizeof(uint32_t), s));
    }
    const fksd::SimArgs* d_launch_args = ctx->args.dev();
    if (batch) {
        /* the previous call has settled, so the pinned staging copies are free */
        HIP_TRY(ctx, ctx->path_args.reserve(records.records));
        fks_batch::build_records(in, *batch, seg_state, seg_done, ctx->path_args.dev(), ctx->path_args.host());
        HIP_TRY(ctx, hipMemcpyAsync(ctx->path_args.dev(), ctx->path_args.host(), records.records * sizeof(fksd::SimArgs),
                                    hipMemcpyHostToDevice, s));
        d_launch_args = ctx->path_args.dev();
    } else {
        fksd::SimArgs& a = *ctx->args.host();
        a = in.base;
        const uint64_t key = splitmix64(in.seed ^ splitmix64(in.call_index));
        a.key0 = (uint32_t)key;
        a.key1 = (uint32_t)(key >> 32);
        a.starts = call.starts;
        a.targets = call.targets;
        a.num_targets = call.num_targets;
        a.n = n;
        a.first_pid = call.first_particle_id;
        a.allow_contacts = call.allow_contacts ? 1 : 0;
        a.out_q = call.out_positions;
        a.pid_io = rq.d_pid_io;
        a.out_collided = call.out_collided;
        a.out_micro = call.out_microsteps;
        a.out_resolver = call.out_resolver_iterations;
        a.out_err = call.out_error_flags;
        fks_batch::apply_segments(plan, &a);
        a.seg_state = seg_state;
        a.seg_done = seg_done;
        if (tr) {
            a.tr_inputs = tr->inputs;
            a.tr_micro = tr->micro;
            a.tr_cfg = tr->cfg;
            a.tr_tags = tr->tags;
            a.tr_nsteps = tr->nsteps;
            a.tr_ncfg = tr->ncfg;
            a.tr_step_cap = tr->step_cap;
            a.tr_cfg_cap = tr->cfg_cap;
        }
        HIP_TRY(ctx, hipMemcpyAsync(ctx->args.dev(), ctx->args.host(), sizeof(a), hipMemcpyHostToDevice, s));
    }
    fks_launch::Request what;
    what.kind = tr ? fks_launch::REQUEST_TRACED : fks_launch::REQUEST_PLAIN;
    if (batch) what = fks_launch::Request{fks_launch::REQUEST_BATCH, batch->form, batch->policy, batch->legs};
    what.n = n;
    what.small = plan.small;
    what.nseg = plan.nseg;
    const fksd::PolicyArgs* pol =
        batch && batch->policy ? reinterpret_cast<const fksd::PolicyArgs*>(ctx->path_args.dev() + records.policy_record) : nullptr;
    return launch_request(ctx, what, d_launch_args, pol, s, rq.synchronize, &ctx->last_kernel);
}

extern "C" {

fks_status fks_forward_simulate_device(fks_context* ctx, const double* d_starts, uint64_t n, const double* d_targets,
                                       uint64_t num_targets, uint64_t first_particle_id, int32_t allow_contacts,
                                       double* d_out_positions, uint8_t* d_out_collided, uint32_t* d_out_microsteps,
                                       uint32_t* d_out_resolver_iterations, uint32_t* d_out_error_flags, void* stream,
                                       int32_t synchronize) {
    SimRequest rq;
    rq.plain = plain_call(d_starts, n, d_targets, num_targets, first_particle_id, allow_contacts, d_out_positions, d_out_collided,
                          d_out_microsteps, d_out_resolver_iterations, d_out_error_flags);
    rq.stream = stream;
    rq.synchronize = synchronize;
    return simulate_device(ctx, rq);
}

fks_status fks_check_config_collision_device(fks_context* ctx, const double* d_configs, uint64_t n, double inflation_ratio,
                                             uint8_t* d_out_collided, uint32_t* d_out_error_flags, void* stream,
                                             int32_t synchronize) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    if (n > 0 && (!d_configs || !d_out_collided)) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "null device buffer");
    if (!(inflation_ratio == inflation_ratio)) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "inflation_ratio is NaN");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ctx->call_start = std::chrono::steady_clock::now();
    std::memset(&ctx->check_last, 0, sizeof(ctx->check_last));
    ctx->check_last.particles = n;
    if (n == 0) return FKS_OK;
    fksd::SimArgs a = base_args(ctx, true);
    /* SPCS:1403-1404 thresholds, SPCS:923 tolerance */
    a.thr_env = (inflation_ratio * ctx->env_g.res) - (ctx->params.environment_collision_check_tolerance * ctx->sdf_g.res);
    a.self_res = (inflation_ratio + 1.0) * ctx->env_g.res;
    a.starts = d_configs;
    a.n = n;
    a.out_collided = d_out_collided;
    a.out_err = d_out_error_flags;
    *ctx->args.host() = a;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->args.dev(), ctx->args.host(), sizeof(a), hipMemcpyHostToDevice, s));
    /* a batch larger than the resident grid builds the robot's module if the simulation has not
     * built it yet (a failure keeps the generic check); the module's shape-specialised check runs
     * whenever the module is there, whatever the batch's size */
    fks_launch::Request what;
    what.kind = fks_launch::REQUEST_CHECK;
    what.n = n;
    return launch_request(ctx, what, ctx->args.dev(), nullptr, s, synchronize, &ctx->last_check_kernel);
}

fks_status fks_check_config_collision(fks_context* ctx, const double* configs, uint64_t n, double inflation_ratio,
                                      uint8_t* out_collided, uint32_t* out_error_flags) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    if (n > 0 && (!configs || !out_collided)) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "null host buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    const size_t W = (size_t)ctx->R.W;
    fks_buf::ParticleStaging& sg = ctx->stage;
    HIP_TRY(ctx, sg.reserve_rows(n, W));
    if (n == 0) return fks_check_config_collision_device(ctx, nullptr, 0, inflation_ratio, nullptr, nullptr, nullptr, 1);
    HIP_TRY(ctx, hipMemcpy(sg.starts.get(), configs, n * W * sizeof(double), hipMemcpyHostToDevice));
    st = fks_check_config_collision_device(ctx, sg.starts.get(), n, inflation_ratio, sg.coll.get(), sg.err.get(), nullptr, 1);
    if (st != FKS_OK) return st;
    HIP_TRY(ctx, sg.download(n, W, nullptr, out_collided, nullptr, nullptr, out_error_flags));
    ctx->check_last.call_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->call_start).count();
    return FKS_OK;
}

fks_status fks_get_last_check_counters(const fks_context* ctx, fks_call_counters* out) {
    if (!ctx || !out) return FKS_ERR_INVALID_ARGUMENT;
    fks_status st = settle(const_cast<fks_context*>(ctx));
    if (st != FKS_OK) return st;
    *out = ctx->check_last;
    return FKS_OK;
}

static fks_status simulate_host(fks_context* ctx, const double* starts, uint64_t n, const double* targets, uint64_t num_targets,
                                int32_t allow_contacts, double* out_positions, uint8_t* out_collided, uint32_t* out_microsteps,
                                uint32_t* out_resolver_iterations, uint32_t* out_error_flags, const TraceDev* tr = nullptr,
                                double* controller_state = nullptr) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    if (n > 0 && (!starts || !targets || !out_positions)) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "null host buffer");
    if (n > 0 && num_targets != 1 && num_targets != n)
        return fail(ctx, FKS_ERR_INVALID_ARGUMENT, fks_batch::kTargetsOneOrN);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    const size_t W = (size_t)ctx->R.W;
    fks_buf::ParticleStaging& sg = ctx->stage;
    HIP_TRY(ctx, sg.reserve_rows(n, W));
    const uint64_t nt = (n > 0) ? num_targets : 0;
    HIP_TRY(ctx, sg.reserve_targets(nt > 0 ? nt : 1, W)); /* one configuration also when there is no particle */
    if (n == 0) {
        ctx->call_index++;
        std::memset(&ctx->last, 0, sizeof(ctx->last));
        return FKS_OK;
    }
    HIP_TRY(ctx, hipMemcpy(sg.starts.get(), starts, n * W * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(sg.targets.get(), targets, nt * W * sizeof(double), hipMemcpyHostToDevice));
    const size_t pid_words = (size_t)n * 2u * (size_t)ctx->R.D;
    if (controller_state) {
        HIP_TRY(ctx, ctx->d_pid.reserve(pid_words));
        HIP_TRY(ctx, hipMemcpy(ctx->d_pid.get(), controller_state, pid_words * sizeof(double), hipMemcpyHostToDevice));
    }
    SimRequest rq;
    rq.plain = plain_call(sg.starts.get(), n, sg.targets.get(), nt, 0, allow_contacts, sg.out.get(), sg.coll.get(), sg.micro.get(),
                          sg.res.get(), sg.err.get());
    rq.trace = tr;
    rq.d_pid_io = controller_state ? ctx->d_pid.get() : nullptr;
    st = simulate_device(ctx, rq);
    if (st != FKS_OK) return st;
    if (controller_state)
        HIP_TRY(ctx, hipMemcpy(controller_state, ctx->d_pid.get(), pid_words * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, sg.download(n, W, out_positions, out_collided, out_microsteps, out_resolver_iterations, out_error_flags));
    ctx->last.call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->call_start).count();
    return FKS_OK;
}

fks_status fks_forward_simulate(fks_context* ctx, const double* starts, uint64_t n, const double* targets, uint64_t num_targets,
                                int32_t allow_contacts, double* out_positions, uint8_t* out_collided, uint32_t* out_microsteps,
                                uint32_t* out_resolver_iterations, uint32_t* out_error_flags) {
    return simulate_host(ctx, starts, n, targets, num_targets, allow_contacts, out_positions, out_collided, out_microsteps,
                         out_resolver_iterations, out_error_flags);
}

/* ReverseSimulateRobots: ReverseSimulateMutableRobot == ForwardSimulateMutableRobot (SPCS:838-841) */
fks_status fks_reverse_simulate(fks_context* ctx, const double* starts, uint64_t n, const double* targets, uint64_t num_targets,
                                int32_t allow_contacts, double* out_positions, uint8_t* out_collided, uint32_t* out_microsteps,
                                uint32_t* out_resolver_iterations, uint32_t* out_error_flags) {
    return simulate_host(ctx, starts, n, targets, num_targets, allow_contacts, out_positions, out_collided, out_microsteps,
                         out_resolver_iterations, out_error_flags);
}

/* ForwardSimulateMutableRobot (SPCS:843-919) over a batch of robots that keep their controllers */
fks_status fks_forward_simulate_mutable(fks_context* ctx, const double* starts, uint64_t n, const double* targets,
                                        uint64_t num_targets, int32_t allow_contacts, double* controller_state,
                                        double* out_positions, uint8_t* out_collided, uint32_t* out_microsteps,
                                        uint32_t* out_resolver_iterations, uint32_t* out_error_flags) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (n > 0 && !controller_state) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "null controller state");
    return simulate_host(ctx, starts, n, targets, num_targets, allow_contacts, out_positions, out_collided, out_microsteps,
                         out_resolver_iterations, out_error_flags, nullptr, controller_state);
}

/* What every batched entry does before anything is staged or counted: the refusals of its
 * arguments (fks_batch::check_arguments) and the plan of its launch on this context */
static fks_status plan_entry(fks_context* ctx, fks_batch::Inputs* in, fks_batch::Batch* b) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    std::string why;
    fks_status st = fks_batch::check_arguments(b, ctx->individual_jacobians != 0, &why);
    if (st == FKS_OK) {
        plan_inputs(ctx, in);
        st = fks_batch::plan_batch(*in, b, &why);
    }
    return st == FKS_OK ? FKS_OK : fail(ctx, st, why);
}

static fks_status run_batch(fks_context* ctx, const fks_batch::Inputs& in, const fks_batch::Batch& b, void* stream,
                            int32_t synchronize) {
    SimRequest rq;
    rq.batch = &b;
    rq.inputs = &in;
    rq.stream = stream;
    rq.synchronize = synchronize;
    return simulate_device(ctx, rq);
}

fks_status fks_forward_simulate_path_device(fks_context* ctx, const double* d_starts, uint64_t n, const double* d_waypoints,
                                            uint64_t num_legs, uint64_t num_targets, uint64_t first_particle_id,
                                            int32_t allow_contacts, double* d_out_positions, uint8_t* d_out_collided,
                                            uint32_t* d_out_microsteps, uint32_t* d_out_resolver_iterations,
                                            uint32_t* d_out_error_flags, void* stream, int32_t synchronize) {
    fks_batch::Inputs in;
    fks_batch::Batch b;
    fks_batch::from_path(&b, fks_batch::ENTRY_PATH_DEVICE, d_starts, n, d_waypoints, num_legs, num_targets, first_particle_id,
                         allow_contacts, d_out_positions, d_out_collided, d_out_microsteps, d_out_resolver_iterations,
                         d_out_error_flags);
    const fks_status st = plan_entry(ctx, &in, &b);
    if (st != FKS_OK) return st;
    return run_batch(ctx, in, b, stream, synchronize);
}

/* Copies straight between the caller's arrays and the staging buffers of the plain host calls
 * (a path's arrays are one block each: the jobs' intermediate host buffer would only add a copy) */
fks_status fks_forward_simulate_path(fks_context* ctx, const double* starts, uint64_t n, const double* waypoints, uint64_t num_legs,
                                     uint64_t num_targets, int32_t allow_contacts, double* out_positions, uint8_t* out_collided,
                                     uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags) {
    fks_batch::Inputs in;
    fks_batch::Batch b;
    fks_batch::from_path(&b, fks_batch::ENTRY_PATH_HOST, starts, n, waypoints, num_legs, num_targets, 0, allow_contacts, out_positions,
                         out_collided, out_microsteps, out_resolver_iterations, out_error_flags);
    fks_status st = plan_entry(ctx, &in, &b);
    if (st != FKS_OK) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = settle(ctx);
    if (st != FKS_OK) return st;
    if (n == 0) return run_batch(ctx, in, b, nullptr, 1);
    /* the staging buffers of the plain host calls, sized for the leg-major outputs */
    const size_t W = (size_t)ctx->R.W;
    const uint64_t rows = n * num_legs, nt = num_targets * num_legs;
    fks_buf::ParticleStaging& sg = ctx->stage;
    HIP_TRY(ctx, sg.reserve_rows(rows, W));
    HIP_TRY(ctx, sg.reserve_targets(nt, W));
    HIP_TRY(ctx, hipMemcpy(sg.starts.get(), starts, n * W * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(sg.targets.get(), waypoints, nt * W * sizeof(double), hipMemcpyHostToDevice));
    fks_path_job& dev = b.converted[0]; /* the same path over the staging buffers */
    dev.starts = sg.starts.get();
    dev.waypoints = sg.targets.get();
    sg.stage_outputs(&dev, 0, W);
    st = run_batch(ctx, in, b, nullptr, 1);
    if (st != FKS_OK) return st;
    HIP_TRY(ctx, sg.download(rows, W, out_positions, out_collided, out_microsteps, out_resolver_iterations, out_error_flags));
    ctx->last.call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->call_start).count();
    return FKS_OK;
}

/* fks_forward_simulate_jobs and _path_jobs over host arrays: the batch's inputs go up in one
 * copy (the staging buffers of the plain host calls: d_starts holds every job's starts and then
 * every job's waypoints), the outputs are the jobs' leg-major blocks one behind the other
 * (b.rows rows; a job's block is one row block), each array comes down in one copy and each
 * job's block goes to its own arrays */
static fks_status simulate_batch_host(fks_context* ctx, const fks_batch::Inputs& in, const fks_batch::Batch& b) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    if (b.total == 0) return run_batch(ctx, in, b, nullptr, 1);
    const size_t W = (size_t)ctx->R.W;
    const uint64_t N = b.total, R = b.rows;
    uint64_t NT = 0;
    for (uint64_t j = 0; j < b.num_jobs; ++j) NT += b.jobs()[j].n > 0 ? b.jobs()[j].num_targets * b.jobs()[j].num_legs : 0;
    fks_buf::ParticleStaging& sg = ctx->stage;
    HIP_TRY(ctx, sg.reserve_rows(std::max(N + NT, R), W)); /* starts also carries the waypoints */
    const size_t in_bytes = (N + NT) * W * sizeof(double);
    ctx->jobs_stage.resize(std::max(in_bytes, fks_buf::HostRows::bytes(R, W)));
    double* h_in = reinterpret_cast<double*>(ctx->jobs_stage.data());
    fks_batch::Batch dev = b; /* the same jobs over the staging buffers */
    dev.converted.assign(b.jobs(), b.jobs() + b.num_jobs);
    uint64_t at = 0, tat = N, oat = 0;
    for (fks_path_job& d : dev.converted) {
        if (d.n == 0) continue;
        const uint64_t nt = d.num_targets * d.num_legs;
        std::memcpy(h_in + at * W, d.starts, d.n * W * sizeof(double));
        std::memcpy(h_in + tat * W, d.waypoints, nt * W * sizeof(double));
        d.starts = sg.starts.get() + at * W;
        d.waypoints = sg.starts.get() + tat * W;
        sg.stage_outputs(&d, oat, W);
        at += d.n;
        tat += nt;
        oat += d.n * d.num_legs;
    }
    HIP_TRY(ctx, hipMemcpy(sg.starts.get(), h_in, in_bytes, hipMemcpyHostToDevice));
    st = run_batch(ctx, in, dev, nullptr, 1);
    if (st != FKS_OK) return st;
    const fks_buf::HostRows h(ctx->jobs_stage.data(), R, W);
    bool want_coll = false, want_micro = false, want_res = false, want_err = false;
    for (uint64_t j = 0; j < b.num_jobs; ++j) {
        const fks_path_job& job = b.jobs()[j];
        if (job.n == 0) continue;
        want_coll |= job.out_collided != nullptr;
        want_micro |= job.out_microsteps != nullptr;
        want_res |= job.out_resolver_iterations != nullptr;
        want_err |= job.out_error_flags != nullptr;
    }
    HIP_TRY(ctx, sg.download(R, W, h.q, want_coll ? h.coll : nullptr, want_micro ? h.micro : nullptr, want_res ? h.res : nullptr,
                             want_err ? h.err : nullptr));
    oat = 0;
    for (uint64_t j = 0; j < b.num_jobs; ++j) {
        const fks_path_job& job = b.jobs()[j];
        if (job.n == 0) continue;
        const uint64_t r = job.n * job.num_legs;
        std::memcpy(job.out_positions, h.q + oat * W, r * W * sizeof(double));
        if (job.out_collided) std::memcpy(job.out_collided, h.coll + oat, r);
        if (job.out_microsteps) std::memcpy(job.out_microsteps, h.micro + oat, r * sizeof(uint32_t));
        if (job.out_resolver_iterations) std::memcpy(job.out_resolver_iterations, h.res + oat, r * sizeof(uint32_t));
        if (job.out_error_flags) std::memcpy(job.out_error_flags, h.err + oat, r * sizeof(uint32_t));
        oat += r;
    }
    ctx->last.call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->call_start).count();
    return FKS_OK;
}

fks_status fks_forward_simulate_policy_device(fks_context* ctx, const double* d_starts, uint64_t n, const fks_policy_table* table,
                                              uint64_t max_legs, uint64_t first_particle_id, int32_t allow_contacts,
                                              double* d_out_positions, uint8_t* d_out_collided, uint32_t* d_out_microsteps,
                                              uint32_t* d_out_resolver_iterations, uint32_t* d_out_error_flags,
                                              uint32_t* d_out_choice, double* d_out_distance, uint32_t* d_out_legs_run,
                                              void* stream, int32_t synchronize) {
    fks_batch::Inputs in;
    fks_batch::Batch b;
    fks_batch::from_policy(&b, fks_batch::ENTRY_POLICY_DEVICE, d_starts, n, table, max_legs, first_particle_id, allow_contacts,
                           d_out_positions, d_out_collided, d_out_microsteps, d_out_resolver_iterations, d_out_error_flags,
                           d_out_choice, d_out_distance, d_out_legs_run);
    const fks_status st = plan_entry(ctx, &in, &b);
    if (st != FKS_OK) return st;
    return run_batch(ctx, in, b, stream, synchronize);
}

/* The table goes up with the starts in one copy (a staging buffer of the roll-out's own, so that a
 * large table grows nothing else: the starts, the keys, the targets, then the flags), the outputs
 * use the path's staging buffers and three of the roll-out's own, and each array comes down in
 * one copy */
fks_status fks_forward_simulate_policy(fks_context* ctx, const double* starts, uint64_t n, const fks_policy_table* table,
                                       uint64_t max_legs, int32_t allow_contacts, double* out_positions, uint8_t* out_collided,
                                       uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags,
                                       uint32_t* out_choice, double* out_distance, uint32_t* out_legs_run) {
    fks_batch::Inputs in;
    fks_batch::Batch b;
    fks_batch::from_policy(&b, fks_batch::ENTRY_POLICY_HOST, starts, n, table, max_legs, 0, allow_contacts, out_positions,
                           out_collided, out_microsteps, out_resolver_iterations, out_error_flags, out_choice, out_distance,
                           out_legs_run);
    fks_status st = plan_entry(ctx, &in, &b);
    if (st != FKS_OK) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = settle(ctx);
    if (st != FKS_OK) return st;
    if (n == 0) return run_batch(ctx, in, b, nullptr, 1);
    const size_t W = (size_t)ctx->R.W;
    const uint64_t M = table->num_entries, rows = n * max_legs, sel = n * (max_legs + 1);
    /* in doubles: starts, keys, targets, flags (two to a double) */
    const uint64_t in_words = (n + 2 * M) * W + (table->flags ? (M + 1) / 2 : 0);
    fks_buf::ParticleStaging& sg = ctx->stage;
    HIP_TRY(ctx, sg.reserve_rows(rows, W));
    HIP_TRY(ctx, ctx->d_policy_in.reserve(in_words)); /* a large table grows this buffer alone */
    HIP_TRY(ctx, ctx->d_policy_choice.reserve(sel));
    HIP_TRY(ctx, ctx->d_policy_distance.reserve(sel));
    HIP_TRY(ctx, ctx->d_policy_legs.reserve(sel)); /* >= n, whatever the next call's legs */
    ctx->jobs_stage.resize(in_words * sizeof(double));
    double* h_in = reinterpret_cast<double*>(ctx->jobs_stage.data());
    std::memcpy(h_in, starts, n * W * sizeof(double));
    std::memcpy(h_in + n * W, table->keys, M * W * sizeof(double));
    std::memcpy(h_in + (n + M) * W, table->targets, M * W * sizeof(double));
    if (table->flags) {
        h_in[in_words - 1] = 0.0; /* the odd entry's other half */
        std::memcpy(h_in + (n + 2 * M) * W, table->flags, M * sizeof(uint32_t));
    }
    double* d_in = ctx->d_policy_in.get();
    HIP_TRY(ctx, hipMemcpy(d_in, h_in, in_words * sizeof(double), hipMemcpyHostToDevice));
    fks_path_job& dev = b.converted[0]; /* the same roll-out over the staging buffers */
    dev.starts = d_in;
    sg.stage_outputs(&dev, 0, W);
    b.table.keys = d_in + n * W;
    b.table.targets = d_in + (n + M) * W;
    b.table.flags = table->flags ? reinterpret_cast<const uint32_t*>(d_in + (n + 2 * M) * W) : nullptr;
    b.out_choice = ctx->d_policy_choice.get();
    b.out_distance = ctx->d_policy_distance.get();
    b.out_legs_run = ctx->d_policy_legs.get();
    st = run_batch(ctx, in, b, nullptr, 1);
    if (st != FKS_OK) return st;
    HIP_TRY(ctx, sg.download(rows, W, out_positions, out_collided, out_microsteps, out_resolver_iterations, out_error_flags));
    HIP_TRY(ctx, hipMemcpy(out_choice, b.out_choice, sel * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_distance) HIP_TRY(ctx, hipMemcpy(out_distance, b.out_distance, sel * sizeof(double), hipMemcpyDeviceToHost));
    if (out_legs_run) HIP_TRY(ctx, hipMemcpy(out_legs_run, b.out_legs_run, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    ctx->last.call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->call_start).count();
    return FKS_OK;
}

/* The clustering launch over device buffers: the offsets and the matrices' prefix go up in one
 * pinned copy on the stream, one workgroup serves a group.  No call index, no counters. */
static fks_status cluster_device(fks_context* ctx, const fks_batch::ClusterPlan& plan, const double* d_configs,
                                 const uint64_t* group_begin, double threshold, double* d_out_distances, uint32_t* d_out_labels,
                                 uint32_t* d_out_num_clusters, hipStream_t s, int32_t synchronize) {
    if (!plan.launch) return FKS_OK;
    const size_t G = (size_t)plan.num_groups, words = 2 * (G + 1);
    HIP_TRY(ctx, ctx->cluster_off.reserve(words));
    if (plan.work_words) HIP_TRY(ctx, ctx->d_cluster_work.reserve((size_t)plan.work_words));
    /* the previous call has settled, so the pinned copy is free */
    std::memcpy(ctx->cluster_off.host(), group_begin, (G + 1) * sizeof(uint64_t));
    std::memcpy(ctx->cluster_off.host() + (G + 1), plan.mat_begin.data(), (G + 1) * sizeof(uint64_t));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->cluster_off.dev(), ctx->cluster_off.host(), words * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    fksd::ClusterArgs a;
    std::memset(&a, 0, sizeof(a));
    a.R = ctx->R;
    a.configs = d_configs;
    a.offsets = ctx->cluster_off.dev();
    a.num_groups = plan.num_groups;
    a.threshold = threshold;
    a.out_distances = d_out_distances;
    a.out_labels = d_out_labels;
    a.out_num_clusters = d_out_num_clusters;
    a.work = plan.work_words ? ctx->d_cluster_work.get() : nullptr;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(plan.num_groups, 1u << 16);
    hipLaunchKernelGGL(kClusterKernels[family_of(ctx->R.type, false)], dim3(grid), dim3(fksd::kClusterThreads), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
    ctx->pending = true;
    ctx->pending_kind = 2;
    ctx->pending_stream = s;
    if (synchronize) return settle(ctx);
    return FKS_OK;
}

/* what both context entries refuse, and the plan of what they run */
static fks_status cluster_entry(fks_context* ctx, fks_batch::ClusterPlan* plan, const double* configs, const uint64_t* group_begin,
                                uint64_t num_groups, double threshold, const void* out_distances, const void* out_labels,
                                const void* out_num_clusters) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    std::string why;
    const fks_status st =
        fks_batch::plan_cluster(plan, configs, group_begin, num_groups, threshold, out_distances, out_labels, out_num_clusters, &why);
    if (st != FKS_OK) return fail(ctx, st, why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return settle(ctx);
}

fks_status fks_cluster_configs_device(fks_context* ctx, const double* d_configs, const uint64_t* group_begin, uint64_t num_groups,
                                      double threshold, double* d_out_distances, uint32_t* d_out_labels,
                                      uint32_t* d_out_num_clusters, void* stream, int32_t synchronize) {
    fks_batch::ClusterPlan plan;
    const fks_status st =
        cluster_entry(ctx, &plan, d_configs, group_begin, num_groups, threshold, d_out_distances, d_out_labels, d_out_num_clusters);
    if (st != FKS_OK) return st;
    return cluster_device(ctx, plan, d_configs, group_begin, threshold, d_out_distances, d_out_labels, d_out_num_clusters,
                          reinterpret_cast<hipStream_t>(stream), synchronize);
}

fks_status fks_cluster_configs_ctx(fks_context* ctx, const double* configs, const uint64_t* group_begin, uint64_t num_groups,
                                   double threshold, double* out_distances, uint32_t* out_labels, uint32_t* out_num_clusters) {
    fks_batch::ClusterPlan plan;
    const fks_status st = cluster_entry(ctx, &plan, configs, group_begin, num_groups, threshold, out_distances, out_labels, out_num_clusters);
    if (st != FKS_OK) return st;
    if (!plan.launch) return FKS_OK;
    const size_t W = (size_t)ctx->R.W, N = (size_t)plan.total, G = (size_t)plan.num_groups;
    const size_t in_words = N * W, mat_words = (size_t)plan.mat_begin[G];
    HIP_TRY(ctx, ctx->d_cluster_in.reserve(in_words));
    if (out_distances) HIP_TRY(ctx, ctx->d_cluster_mat.reserve(mat_words));
    if (out_labels) HIP_TRY(ctx, ctx->d_cluster_labels.reserve(N));
    if (out_num_clusters) HIP_TRY(ctx, ctx->d_cluster_counts.reserve(G));
    double* d_mat = out_distances ? ctx->d_cluster_mat.get() : nullptr;
    uint32_t* d_labels = out_labels ? ctx->d_cluster_labels.get() : nullptr;
    uint32_t* d_counts = out_num_clusters ? ctx->d_cluster_counts.get() : nullptr;
    /* configs [N][W] goes up in one copy */
    if (in_words && configs) HIP_TRY(ctx, hipMemcpy(ctx->d_cluster_in.get(), configs, in_words * sizeof(double), hipMemcpyHostToDevice));
    const fks_status run = cluster_device(ctx, plan, ctx->d_cluster_in.get(), group_begin, threshold, d_mat, d_labels, d_counts, nullptr, 1);
    if (run != FKS_OK) return run;
    if (d_mat && mat_words) HIP_TRY(ctx, hipMemcpy(out_distances, d_mat, mat_words * sizeof(double), hipMemcpyDeviceToHost));
    /* labels before group_begin[0] belong to no group: the caller's stay as they are */
    const size_t first = (size_t)group_begin[0];
    if (d_labels && N > first)
        HIP_TRY(ctx, hipMemcpy(out_labels + first, d_labels + first, (N - first) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (d_counts) HIP_TRY(ctx, hipMemcpy(out_num_clusters, d_counts, G * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FKS_OK;
}

/* The summary launch over device buffers: the offsets go up in one pinned copy on the stream, one
 * workgroup serves a group.  No call index, no counters. */
static fks_status summary_device(fks_context* ctx, const fks_batch::SummaryPlan& plan, const double* d_configs,
                                 const uint64_t* group_begin, const uint32_t* d_labels, const double* d_targets,
                                 double reached_distance, const fks_cluster_summary& d_out, hipStream_t s, int32_t synchronize) {
    if (!plan.launch) return FKS_OK;
    const size_t words = (size_t)plan.num_groups + 1;
    HIP_TRY(ctx, ctx->summary_off.reserve(words));
    HIP_TRY(ctx, ctx->d_summary_work.reserve((size_t)plan.work_words));
    /* the previous call has settled, so the pinned copy is free */
    std::memcpy(ctx->summary_off.host(), group_begin, words * sizeof(uint64_t));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->summary_off.dev(), ctx->summary_off.host(), words * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    fksd::SummaryArgs a;
    std::memset(&a, 0, sizeof(a));
    a.R = ctx->R;
    a.configs = d_configs;
    a.offsets = ctx->summary_off.dev();
    a.labels = d_labels;
    a.targets = d_targets;
    a.num_groups = plan.num_groups;
    a.total = plan.total;
    a.reached_distance = reached_distance;
    a.piece_width = plan.piece_width;
    a.work = ctx->d_summary_work.get();
    a.out_order = d_out.order;
    a.out_members = d_out.members;
    a.out_count = d_out.count;
    a.out_begin = d_out.begin;
    a.out_expectation = d_out.expectation;
    a.out_variances = d_out.variances;
    a.out_variance = d_out.variance;
    a.out_reached = d_out.reached;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(plan.num_groups, 1u << 16);
    hipLaunchKernelGGL(kSummaryKernels[family_of(ctx->R.type, false)], dim3(grid), dim3(fksd::kSummaryThreads), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
    ctx->pending = true;
    ctx->pending_kind = 2;
    ctx->pending_stream = s;
    if (synchronize) return settle(ctx);
    return FKS_OK;
}

/* what both context entries refuse, and the plan of what they run */
static fks_status summary_entry(fks_context* ctx, fks_batch::SummaryPlan* plan, const double* configs, const uint64_t* group_begin,
                                uint64_t num_groups, const uint32_t* labels, const double* targets, double reached_distance,
                                const fks_cluster_summary* out) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    std::string why;
    const fks_status st = fks_batch::plan_summary(plan, ctx->R.type, (uint32_t)ctx->R.W, configs, group_begin, num_groups, labels,
                                                  targets, reached_distance, out, &why);
    if (st != FKS_OK) return fail(ctx, st, why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return settle(ctx);
}

fks_status fks_summarize_clusters_device(fks_context* ctx, const double* d_configs, const uint64_t* group_begin, uint64_t num_groups,
                                         const uint32_t* d_labels, const double* d_targets, double reached_distance,
                                         const fks_cluster_summary* d_out, void* stream, int32_t synchronize) {
    fks_batch::SummaryPlan plan;
    const fks_status st = summary_entry(ctx, &plan, d_configs, group_begin, num_groups, d_labels, d_targets, reached_distance, d_out);
    if (st != FKS_OK) return st;
    return summary_device(ctx, plan, d_configs, group_begin, d_labels, d_targets, reached_distance, *d_out,
                          reinterpret_cast<hipStream_t>(stream), synchronize);
}

fks_status fks_summarize_clusters_ctx(fks_context* ctx, const double* configs, const uint64_t* group_begin, uint64_t num_groups,
                                      const uint32_t* labels, const double* targets, double reached_distance,
                                      const fks_cluster_summary* out) {
    fks_batch::SummaryPlan plan;
    const fks_status st = summary_entry(ctx, &plan, configs, group_begin, num_groups, labels, targets, reached_distance, out);
    if (st != FKS_OK) return st;
    if (!plan.launch) return FKS_OK;
    const size_t W = plan.width, Wv = plan.var_width, N = (size_t)plan.total, G = (size_t)plan.num_groups;
    /* the doubles: configs [N][W], targets [G][W], then members, expectation [N][W], variances [N][Wv], variance [N] */
    const size_t f_targets = N * W, f_members = f_targets + (targets ? G * W : 0), f_expect = f_members + (out->members ? N * W : 0),
                 f_vars = f_expect + (out->expectation ? N * W : 0), f_var = f_vars + (out->variances ? N * Wv : 0),
                 f_end = f_var + (out->variance ? N : 0);
    /* the words: labels [N], then order, count, begin, reached [N] */
    const size_t u_order = N, u_count = u_order + (out->order ? N : 0), u_begin = u_count + (out->count ? N : 0),
                 u_reached = u_begin + (out->begin ? N : 0), u_end = u_reached + (out->reached ? N : 0);
    HIP_TRY(ctx, ctx->d_summary_f64.reserve(f_end));
    HIP_TRY(ctx, ctx->d_summary_u32.reserve(u_end));
    double* df = ctx->d_summary_f64.get();
    uint32_t* du = ctx->d_summary_u32.get();
    fks_cluster_summary d;
    d.order = out->order ? du + u_order : nullptr;
    d.count = out->count ? du + u_count : nullptr;
    d.begin = out->begin ? du + u_begin : nullptr;
    d.reached = out->reached ? du + u_reached : nullptr;
    d.members = out->members ? df + f_members : nullptr;
    d.expectation = out->expectation ? df + f_expect : nullptr;
    d.variances = out->variances ? df + f_vars : nullptr;
    d.variance = out->variance ? df + f_var : nullptr;
    /* rows below group_begin[0] belong to no group: nothing of theirs goes up or comes down */
    const size_t first = (size_t)plan.first, rows = N - first;
    if (rows) {
        HIP_TRY(ctx, hipMemcpy(df + first * W, configs + first * W, rows * W * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(du + first, labels + first, rows * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (targets && G) HIP_TRY(ctx, hipMemcpy(df + f_targets, targets, G * W * sizeof(double), hipMemcpyHostToDevice));
    const fks_status run = summary_device(ctx, plan, df, group_begin, du, targets ? df + f_targets : nullptr, reached_distance, d, nullptr, 1);
    if (run != FKS_OK) return run;
    if (!rows) return FKS_OK;
    auto down_f = [&](double* host, const double* dev, size_t width) {
        return host ? hipMemcpy(host + first * width, dev + first * width, rows * width * sizeof(double), hipMemcpyDeviceToHost) : hipSuccess;
    };
    auto down_u = [&](uint32_t* host, const uint32_t* dev) {
        return host ? hipMemcpy(host + first, dev + first, rows * sizeof(uint32_t), hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIP_TRY(ctx, down_u(out->order, d.order));
    HIP_TRY(ctx, down_f(out->members, d.members, W));
    HIP_TRY(ctx, down_u(out->count, d.count));
    HIP_TRY(ctx, down_u(out->begin, d.begin));
    HIP_TRY(ctx, down_f(out->expectation, d.expectation, W));
    HIP_TRY(ctx, down_f(out->variances, d.variances, Wv));
    HIP_TRY(ctx, down_f(out->variance, d.variance, 1));
    HIP_TRY(ctx, down_u(out->reached, d.reached));
    return FKS_OK;
}

/* The selection's two launches over device buffers, on one stream with nothing coming down in between: the search
 * (one workgroup per query tile and chunk of states) and the draw (one workgroup per query), which is launched
 * for a single chunk too.  No call index, no counters. */
static fks_status select_device(fks_context* ctx, const fks_batch::SelectPlan& plan, const fks_state_table& d_table,
                                const double* d_queries, uint64_t draw_seed, const fks_state_selection& d_out, hipStream_t s,
                                int32_t synchronize) {
    if (!plan.launch) return FKS_OK;
    HIP_TRY(ctx, ctx->d_select_partials.reserve((size_t)plan.work_partials));
    const uint64_t key = splitmix64(draw_seed);
    fksd::SelectArgs a;
    std::memset(&a, 0, sizeof(a));
    a.R = ctx->R;
    a.keys = d_table.keys;
    a.weights = d_table.weights;
    a.count = d_table.count;
    a.begin = d_table.begin;
    a.members = d_table.members;
    a.num_states = plan.num_states;
    a.num_member_rows = d_table.num_member_rows;
    a.queries = d_queries;
    a.num_queries = plan.num_queries;
    a.particles = plan.draw ? plan.particles : 0u;
    a.k0 = (uint32_t)key;
    a.k1 = (uint32_t)(key >> 32);
    a.chunk_states = plan.chunk_states;
    a.chunks = plan.chunks;
    a.partials = ctx->d_select_partials.get();
    a.out_choice = d_out.choice;
    a.out_distance = d_out.distance;
    a.out_starts = d_out.starts;
    a.out_source = d_out.source;
    void (*kernel)(const fksd::SelectArgs) = ctx->R.type == FKS_ROBOT_LINKED
                                                 ? fks_state_select_linked
                                                 : (ctx->R.type == FKS_ROBOT_SE2 ? fks_state_select_se2 : fks_state_select_se3);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)plan.groups), dim3(fksd::kSelectThreads), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fks_state_draw, dim3((uint32_t)plan.num_queries), dim3(fksd::kSelectThreads), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
    ctx->pending = true;
    ctx->pending_kind = 2;
    ctx->pending_stream = s;
    if (synchronize) return settle(ctx);
    return FKS_OK;
}

/* what both context entries refuse, and the plan of what they run */
static fks_status select_entry(fks_context* ctx, fks_batch::SelectPlan* plan, const fks_state_table* table, const double* queries,
                               uint64_t num_queries, uint32_t num_particles, const fks_state_selection* out) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    if (ctx->compute_units == 0)
        HIP_TRY(ctx, hipDeviceGetAttribute(&ctx->compute_units, hipDeviceAttributeMultiprocessorCount, ctx->device));
    std::string why;
    const fks_status st = fks_batch::plan_select(plan, (uint32_t)ctx->R.W, ctx->compute_units, table, queries, num_queries,
                                                 num_particles, out, &why);
    if (st != FKS_OK) return fail(ctx, st, why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return settle(ctx);
}

fks_status fks_select_states_device(fks_context* ctx, const fks_state_table* d_table, const double* d_queries, uint64_t num_queries,
                                    uint32_t num_particles, uint64_t draw_seed, const fks_state_selection* d_out, void* stream,
                                    int32_t synchronize) {
    fks_batch::SelectPlan plan;
    const fks_status st = select_entry(ctx, &plan, d_table, d_queries, num_queries, num_particles, d_out);
    if (st != FKS_OK) return st;
    return select_device(ctx, plan, *d_table, d_queries, draw_seed, *d_out, reinterpret_cast<hipStream_t>(stream), synchronize);
}

fks_status fks_select_states_ctx(fks_context* ctx, const fks_state_table* table, const double* queries, uint64_t num_queries,
                                 uint32_t num_particles, uint64_t draw_seed, const fks_state_selection* out) {
    fks_batch::SelectPlan plan;
    const fks_status st = select_entry(ctx, &plan, table, queries, num_queries, num_particles, out);
    if (st != FKS_OK) return st;
    if (!plan.launch) return FKS_OK;
    const size_t W = plan.width, S = (size_t)plan.num_states, J = (size_t)plan.num_queries, P = plan.particles;
    const size_t rows = plan.draw ? (size_t)table->num_member_rows : 0;
    auto words = [](size_t n) { return (n + 1) / 2; }; /* doubles that hold n 32-bit words */
    /* the inputs, in doubles from the staging's start: keys, queries, weights, members, count, begin; then the outputs */
    const size_t i_keys = 0, i_queries = i_keys + S * W, i_weights = i_queries + J * W, i_members = i_weights + (table->weights ? S : 0),
                 i_count = i_members + rows * W, i_begin = i_count + (table->count ? words(S) : 0),
                 i_end = i_begin + (table->begin ? words(S) : 0);
    const size_t o_choice = i_end, o_distance = o_choice + words(J), o_starts = o_distance + (out->distance ? J : 0),
                 o_source = o_starts + (out->starts ? J * P * W : 0), o_end = o_source + (out->source ? words(J * P) : 0);
    HIP_TRY(ctx, ctx->d_select_stage.reserve(o_end));
    ctx->select_stage.resize(i_end);
    double* h = ctx->select_stage.data();
    std::memcpy(h + i_keys, table->keys, S * W * sizeof(double));
    std::memcpy(h + i_queries, queries, J * W * sizeof(double));
    if (table->weights) std::memcpy(h + i_weights, table->weights, S * sizeof(double));
    if (rows) std::memcpy(h + i_members, table->members, rows * W * sizeof(double));
    if (table->count) std::memcpy(h + i_count, table->count, S * sizeof(uint32_t));
    if (table->begin) std::memcpy(h + i_begin, table->begin, S * sizeof(uint32_t));
    double* d = ctx->d_select_stage.get();
    HIP_TRY(ctx, hipMemcpy(d, h, i_end * sizeof(double), hipMemcpyHostToDevice));
    fks_state_table dt = *table;
    dt.keys = d + i_keys;
    dt.weights = table->weights ? d + i_weights : nullptr;
    dt.members = table->members ? d + i_members : nullptr;
    dt.count = table->count ? reinterpret_cast<const uint32_t*>(d + i_count) : nullptr;
    dt.begin = table->begin ? reinterpret_cast<const uint32_t*>(d + i_begin) : nullptr;
    /* members that are given but not drawn from are not staged, and then not named either */
    if (!plan.draw) dt.members = nullptr;
    fks_state_selection ds;
    ds.choice = reinterpret_cast<uint32_t*>(d + o_choice);
    ds.distance = out->distance ? d + o_distance : nullptr;
    ds.starts = out->starts ? d + o_starts : nullptr;
    ds.source = out->source ? reinterpret_cast<uint32_t*>(d + o_source) : nullptr;
    const fks_status run = select_device(ctx, plan, dt, d + i_queries, draw_seed, ds, nullptr, 1);
    if (run != FKS_OK) return run;
    HIP_TRY(ctx, hipMemcpy(out->choice, ds.choice, J * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out->distance) HIP_TRY(ctx, hipMemcpy(out->distance, ds.distance, J * sizeof(double), hipMemcpyDeviceToHost));
    if (out->starts) HIP_TRY(ctx, hipMemcpy(out->starts, ds.starts, J * P * W * sizeof(double), hipMemcpyDeviceToHost));
    if (out->source) HIP_TRY(ctx, hipMemcpy(out->source, ds.source, J * P * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FKS_OK;
}

fks_status fks_forward_simulate_jobs_device(fks_context* ctx, const fks_job* jobs, uint64_t num_jobs, void* stream,
                                            int32_t synchronize) {
    fks_batch::Inputs in;
    fks_batch::Batch b;
    fks_batch::from_jobs(&b, jobs, num_jobs);
    const fks_status st = plan_entry(ctx, &in, &b);
    if (st != FKS_OK) return st;
    return run_batch(ctx, in, b, stream, synchronize);
}

fks_status fks_forward_simulate_jobs(fks_context* ctx, const fks_job* jobs, uint64_t num_jobs) {
    fks_batch::Inputs in;
    fks_batch::Batch b;
    fks_batch::from_jobs(&b, jobs, num_jobs);
    const fks_status st = plan_entry(ctx, &in, &b);
    if (st != FKS_OK) return st;
    return simulate_batch_host(ctx, in, b);
}

fks_status fks_forward_simulate_path_jobs_device(fks_context* ctx, const fks_path_job* jobs, uint64_t num_jobs, void* stream,
                                                 int32_t synchronize) {
    fks_batch::Inputs in;
    fks_batch::Batch b;
    fks_batch::from_path_jobs(&b, jobs, num_jobs);
    const fks_status st = plan_entry(ctx, &in, &b);
    if (st != FKS_OK) return st;
    return run_batch(ctx, in, b, stream, synchronize);
}

fks_status fks_forward_simulate_path_jobs(fks_context* ctx, const fks_path_job* jobs, uint64_t num_jobs) {
    fks_batch::Inputs in;
    fks_batch::Batch b;
    fks_batch::from_path_jobs(&b, jobs, num_jobs);
    const fks_status st = plan_entry(ctx, &in, &b);
    if (st != FKS_OK) return st;
    return simulate_batch_host(ctx, in, b);
}

}  // extern "C"

/* a block of `count` elements, all zero (a trace's records past a particle's count stay zero, as
 * in the caller's view) */
template <typename T>
static hipError_t zeroed(DeviceBuffer<T>& b, size_t count) {
    const hipError_t e = b.reserve(count);
    return e != hipSuccess ? e : hipMemset(b.get(), 0, b.capacity() * sizeof(T));
}

/* the traced calls: device trace buffers around simulate_host, copied to the caller's */
static fks_status simulate_traced(fks_context* ctx, const double* starts, uint64_t n, const double* targets, uint64_t num_targets,
                                  int32_t allow_contacts, double* controller_state, double* out_positions, uint8_t* out_collided,
                                  uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags,
                                  const fks_trace* trace) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    if (!trace || !trace->num_steps || !trace->num_configs ||
        (trace->step_capacity > 0 && (!trace->step_inputs || !trace->step_microsteps)) ||
        (trace->config_capacity > 0 && (!trace->configs || !trace->config_tags)))
        return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "incomplete fks_trace");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t D = (size_t)ctx->R.D, W = (size_t)ctx->R.W;
    const size_t ns = (size_t)n * trace->step_capacity, nc = (size_t)n * trace->config_capacity;
    /* the call's own buffers, given back when it returns */
    DeviceBuffer<double> d_inputs, d_cfg;
    DeviceBuffer<uint32_t> d_micro, d_tags, d_nsteps, d_ncfg;
    hipError_t e = zeroed(d_inputs, ns * 2 * D);
    if (e == hipSuccess) e = zeroed(d_micro, ns);
    if (e == hipSuccess) e = zeroed(d_cfg, nc * W);
    if (e == hipSuccess) e = zeroed(d_tags, nc * 3);
    if (e == hipSuccess) e = zeroed(d_nsteps, (size_t)n);
    if (e == hipSuccess) e = zeroed(d_ncfg, (size_t)n);
    if (e != hipSuccess) return hip_fail(ctx, e, "trace buffers");
    const TraceDev tr = {d_inputs.get(), d_micro.get(), d_cfg.get(),          d_tags.get(),
                         d_nsteps.get(), d_ncfg.get(),  trace->step_capacity, trace->config_capacity};
    fks_status st = simulate_host(ctx, starts, n, targets, num_targets, allow_contacts, out_positions, out_collided,
                                  out_microsteps, out_resolver_iterations, out_error_flags, &tr, controller_state);
    if (st == FKS_OK && n > 0) {
        struct Copy {
            void* dst;
            const void* src;
            size_t bytes;
        } copies[] = {{trace->step_inputs, tr.inputs, ns * 2 * D * sizeof(double)},
                      {trace->step_microsteps, tr.micro, ns * sizeof(uint32_t)},
                      {trace->configs, tr.cfg, nc * W * sizeof(double)},
                      {trace->config_tags, tr.tags, nc * 3 * sizeof(uint32_t)},
                      {trace->num_steps, tr.nsteps, (size_t)n * sizeof(uint32_t)},
                      {trace->num_configs, tr.ncfg, (size_t)n * sizeof(uint32_t)}};
        for (const Copy& c : copies) {
            if (c.bytes == 0) continue;
            e = hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                st = hip_fail(ctx, e, "trace copy");
                break;
            }
        }
    }
    return st;
}

extern "C" {

/* ForwardSimulateRobot with enable_tracing = true (SPCS:824-829), batched */
fks_status fks_forward_simulate_traced(fks_context* ctx, const double* starts, uint64_t n, const double* targets,
                                       uint64_t num_targets, int32_t allow_contacts, double* out_positions,
                                       uint8_t* out_collided, uint32_t* out_microsteps, uint32_t* out_resolver_iterations,
                                       uint32_t* out_error_flags, const fks_trace* trace) {
    return simulate_traced(ctx, starts, n, targets, num_targets, allow_contacts, nullptr, out_positions, out_collided,
                           out_microsteps, out_resolver_iterations, out_error_flags, trace);
}

/* ForwardSimulateMutableRobot with enable_tracing = true (SPCS:843-919) */
fks_status fks_forward_simulate_traced_mutable(fks_context* ctx, const double* starts, uint64_t n, const double* targets,
                                               uint64_t num_targets, int32_t allow_contacts, double* controller_state,
                                               double* out_positions, uint8_t* out_collided, uint32_t* out_microsteps,
                                               uint32_t* out_resolver_iterations, uint32_t* out_error_flags,
                                               const fks_trace* trace) {
    if (ctx && n > 0 && !controller_state) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "null controller state");
    return simulate_traced(ctx, starts, n, targets, num_targets, allow_contacts, controller_state, out_positions, out_collided,
                           out_microsteps, out_resolver_iterations, out_error_flags, trace);
}

fks_status fks_robot_sizes(const fks_context* ctx, int32_t* num_links, int32_t* num_points, int32_t* num_dofs,
                           int32_t* config_width) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return FKS_ERR_NO_ROBOT;
    if (num_links) *num_links = ctx->R.L;
    if (num_points) *num_points = ctx->R.P;
    if (num_dofs) *num_dofs = ctx->R.D;
    if (config_width) *config_width = ctx->R.W;
    return FKS_OK;
}

/* FK / world points / clean control input of a batch (include/fks_capi.h) */
fks_status fks_kinematics(fks_context* ctx, int32_t mode, const double* configs, uint64_t n, const double* inputs,
                          double* out) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    if (mode != FKS_KIN_LINK_TRANSFORMS && mode != FKS_KIN_POINTS && mode != FKS_KIN_APPLY_CONTROL_INPUT)
        return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "unknown kinematics mode");
    if (n > 0 && (!configs || !out || (mode == FKS_KIN_APPLY_CONTROL_INPUT && !inputs)))
        return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "null host buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    if (n == 0) return FKS_OK;
    const size_t W = (size_t)ctx->R.W, D = (size_t)ctx->R.D;
    const size_t per_out = (mode == FKS_KIN_LINK_TRANSFORMS) ? 12 * (size_t)ctx->R.L
                                                             : (mode == FKS_KIN_POINTS ? 3 * (size_t)ctx->R.P : W);
    DeviceBuffer<double> d_cfg, d_in, d_out; /* the call's own, given back when it returns */
    hipError_t e = upload(d_cfg, configs, (size_t)n * W);
    if (e == hipSuccess && mode == FKS_KIN_APPLY_CONTROL_INPUT) e = upload(d_in, inputs, (size_t)n * D);
    if (e == hipSuccess) e = d_out.reserve((size_t)n * per_out);
    if (e != hipSuccess) return hip_fail(ctx, e, "kinematics buffers");
    fksd::SimArgs a = base_args(ctx, false);
    a.starts = d_cfg.get();
    a.targets = d_in.get();
    a.n = n;
    a.kin_mode = mode;
    a.kin_out = d_out.get();
    *ctx->args.host() = a;
    e = hipMemcpy(ctx->args.dev(), ctx->args.host(), sizeof(a), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const fks_launch::Geometry g = fks_launch::launch_geometry(ctx->lay, n);
        const KernelId id{fks_launch::KINEMATICS, fks_launch::THROUGHPUT, family_of(ctx->R.type, ctx->lay.lean)};
        const sim_kernel_t k = sim_kernel_of(id);
        if (!k) return fail(ctx, FKS_ERR_UNSUPPORTED, "no kinematics kernel for this robot");
        hipLaunchKernelGGL(k, dim3(g.blocks), dim3(g.threads), g.lds_bytes, nullptr,
                           static_cast<const fksd::SimArgs*>(ctx->args.dev()));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out.get(), (size_t)n * per_out * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(ctx, e, "fks_kinematics");
    return FKS_OK;
}

fks_status fks_set_call_index(fks_context* ctx, uint64_t call_index) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    ctx->call_index = call_index;
    return FKS_OK;
}
uint64_t fks_get_call_index(const fks_context* ctx) { return ctx ? ctx->call_index : 0; }

fks_status fks_get_statistics(const fks_context* ctx, fks_statistics* out) {
    if (!ctx || !out) return FKS_ERR_INVALID_ARGUMENT;
    fks_status st = settle(const_cast<fks_context*>(ctx));
    if (st != FKS_OK) return st;
    *out = ctx->stats;
    return FKS_OK;
}
fks_status fks_reset_statistics(fks_context* ctx) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    std::memset(&ctx->stats, 0, sizeof(ctx->stats));
    return FKS_OK;
}
fks_status fks_set_statistics(fks_context* ctx, const fks_statistics* stats) {
    if (!ctx || !stats) return FKS_ERR_INVALID_ARGUMENT;
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    ctx->stats = *stats;
    return FKS_OK;
}
fks_status fks_reset_generators(fks_context* ctx, uint64_t prng_seed) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    ctx->seed = prng_seed;
    ctx->call_index = 0;
    return FKS_OK;
}
int32_t fks_get_debug_level(const fks_context* ctx) { return ctx ? ctx->debug_level : 0; }
int32_t fks_set_debug_level(fks_context* ctx, int32_t debug_level) {
    if (!ctx) return 0;
    ctx->debug_level = debug_level;
    return ctx->debug_level;
}
fks_status fks_get_last_call_counters(const fks_context* ctx, fks_call_counters* out) {
    if (!ctx || !out) return FKS_ERR_INVALID_ARGUMENT;
    fks_status st = settle(const_cast<fks_context*>(ctx));
    if (st != FKS_OK) return st;
    *out = ctx->last;
    return FKS_OK;
}

fks_status fks_get_total_counters(const fks_context* ctx, fks_call_counters* out) {
    if (!ctx || !out) return FKS_ERR_INVALID_ARGUMENT;
    fks_status st = settle(const_cast<fks_context*>(ctx));
    if (st != FKS_OK) return st;
    *out = ctx->total;
    return FKS_OK;
}
fks_status fks_set_total_counters(fks_context* ctx, const fks_call_counters* totals) {
    if (!ctx || !totals) return FKS_ERR_INVALID_ARGUMENT;
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    ctx->total = *totals;
    return FKS_OK;
}
fks_status fks_reset_total_counters(fks_context* ctx) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    std::memset(&ctx->total, 0, sizeof(ctx->total));
    std::memset(ctx->phase_total, 0, sizeof(ctx->phase_total));
    return FKS_OK;
}

fks_status fks_get_phase_cycles(const fks_context* ctx, int which, uint64_t* out) {
    if (!ctx || !out || (which != 0 && which != 1)) return FKS_ERR_INVALID_ARGUMENT;
    fks_status st = settle(const_cast<fks_context*>(ctx));
    if (st != FKS_OK) return st;
    std::memcpy(out, which ? ctx->phase_total : ctx->phase_last, sizeof(ctx->phase_last));
    return FKS_OK;
}

fks_status fks_set_segment_steps(fks_context* ctx, uint32_t controller_steps) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    ctx->segment_steps = controller_steps;
    return FKS_OK;
}

fks_status fks_set_small_batch_kernel(fks_context* ctx, int32_t enabled) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    ctx->small_batch = enabled ? 1 : 0;
    return FKS_OK;
}

fks_status fks_set_cooperative_waves(fks_context* ctx, int32_t enabled) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    ctx->cooperative = enabled ? 1 : 0;
    return FKS_OK;
}

fks_status fks_set_segment_heavy_relative(fks_context* ctx, uint32_t times_mean) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (times_mean > 64u) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "times_mean must be at most 64");
    ctx->heavy_relative = times_mean;
    return FKS_OK;
}

fks_status fks_set_segment_policy(fks_context* ctx, uint32_t heavy_resolver_per_step, uint32_t heavy_priority) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (heavy_resolver_per_step > 65536u) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "heavy_resolver_per_step > 65536");
    if (heavy_priority > 2u) return fail(ctx, FKS_ERR_INVALID_ARGUMENT, "heavy_priority must be 0, 1 or 2");
    ctx->heavy_per_step = heavy_resolver_per_step;
    ctx->heavy_priority = heavy_priority;
    return FKS_OK;
}

fks_status fks_set_individual_jacobians(fks_context* ctx, int32_t simulate_with_individual_jacobians) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    ctx->individual_jacobians = simulate_with_individual_jacobians ? 1 : 0;
    return FKS_OK;
}

fks_status fks_set_specialization(fks_context* ctx, int32_t mode) {
    if (!ctx || mode < FKS_SPECIALIZE_OFF || mode > FKS_SPECIALIZE_NO_PROOFS) return FKS_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    ctx->specialize = mode;
    ctx->spec.pending = false;
    /* the batched module is released with the plain one and, when the mode allows it, built
     * again at the first batch that runs it (or by fks_prepare_batched_specialization): this
     * call compiles the plain module only */
    shaped_release(ctx, &ctx->bspec);
    ctx->bspec.pending = mode == FKS_SPECIALIZE_ON && ctx->has_robot;
    return shaped_prepare(ctx, &ctx->spec, kPlainModule); /* now, for the current robot (releases it when disabled) */
}

fks_status fks_prepare_batched_specialization(fks_context* ctx) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return fail(ctx, FKS_ERR_NO_ROBOT, "fks_set_robot has not been called");
    if (ctx->specialize != FKS_SPECIALIZE_ON)
        return fail(ctx, FKS_ERR_UNSUPPORTED, "the batched module needs fks_set_specialization(ctx, FKS_SPECIALIZE_ON)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const fks_status st = settle(ctx);
    if (st != FKS_OK) return st;
    ctx->bspec_enabled = 1;
    ctx->bspec.pending = false;
    if (ctx->bspec.fn) return FKS_OK; /* built already */
    return shaped_prepare(ctx, &ctx->bspec, kBatchedModule);
}

fks_status fks_set_batched_specialization(fks_context* ctx, int32_t enabled) {
    if (!ctx) return FKS_ERR_INVALID_ARGUMENT;
    ctx->bspec_enabled = enabled ? 1 : 0;
    return FKS_OK;
}

static fks_status shaped_info(fks_specialization_info* out, int32_t enabled, bool pending, const ShapedModule& m) {
    std::memset(out, 0, sizeof(*out));
    out->enabled = enabled;
    out->active = m.fn ? 1 : 0;
    out->pending = pending ? 1 : 0;
    out->from_cache = m.from_cache;
    out->compile_seconds = m.seconds;
    out->launches = m.launches;
    std::snprintf(out->shape, sizeof(out->shape), "%s", m.shape.c_str());
    out->failed = m.failed ? 1 : 0;
    std::snprintf(out->message, sizeof(out->message), "%s", m.message.c_str());
    return FKS_OK;
}

fks_status fks_get_batched_specialization(const fks_context* ctx, fks_specialization_info* out) {
    if (!ctx || !out) return FKS_ERR_INVALID_ARGUMENT;
    return shaped_info(out, ctx->bspec_enabled, ctx->bspec.pending && ctx->bspec_enabled, ctx->bspec);
}

fks_status fks_get_specialization(const fks_context* ctx, fks_specialization_info* out) {
    if (!ctx || !out) return FKS_ERR_INVALID_ARGUMENT;
    return shaped_info(out, ctx->specialize, ctx->spec.pending, ctx->spec);
}

fks_status fks_get_launch_geometry(const fks_context* ctx, uint32_t* resident_waves, uint64_t* lds_bytes_per_group) {
    if (!ctx || !resident_waves || !lds_bytes_per_group) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return FKS_ERR_NO_ROBOT;
    *resident_waves = ctx->lay.grid_waves;
    *lds_bytes_per_group = (uint64_t)ctx->lay.lds_bytes;
    return FKS_OK;
}

fks_status fks_get_launch_info(const fks_context* ctx, fks_launch_info* out) {
    if (!ctx || !out) return FKS_ERR_INVALID_ARGUMENT;
    if (!ctx->has_robot) return FKS_ERR_NO_ROBOT;
    std::memset(out, 0, sizeof(*out));
    out->resident_waves = ctx->lay.grid_waves;
    out->waves_per_group = ctx->lay.waves_per_group;
    out->lds_bytes_per_group = (uint64_t)ctx->lay.lds_bytes;
    out->small_batch_resident_waves = ctx->lay.small_grid_waves;
    out->standard_layout_resident_waves = ctx->lay.standard_resident_waves;
    out->fk_pair = ctx->lay.fk_pair ? 1 : 0;
    out->lean = ctx->lay.lean ? 1 : 0;
    out->last_kernel = ctx->last_kernel;
    out->last_check_kernel = ctx->last_check_kernel;
    out->cooperative_resident_particles = ctx->lay.coop_particles;
    out->cooperative_waves_per_particle = ctx->lay.coop_waves;
    return FKS_OK;
}

fks_status fks_selftest_math(int32_t device, uint64_t n, uint64_t* out_mismatches) {
    if (!out_mismatches || n == 0 || n > (1ull << 26)) return FKS_ERR_INVALID_ARGUMENT;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return FKS_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return FKS_ERR_HIP;
    std::vector<double> a(n), b(n), host(8 * n), dev(8 * n);
    uint64_t st = 0x1234567ull;
    for (uint64_t i = 0; i < n; ++i) {
        st = splitmix64(st);
        a[i] = ((double)(st >> 11) * (1.0 / 9007199254740992.0) - 0.5) * 40.0;
        st = splitmix64(st);
        b[i] = ((double)(st >> 11) * (1.0 / 9007199254740992.0) - 0.5) * std::pow(10.0, (double)((st & 15) - 6));
    }
    for (uint64_t i = 0; i < n; ++i) {
        const double x = a[i], y = b[i];
        host[8 * i + 0] = fks_math::sin(x);
        host[8 * i + 1] = fks_math::cos(x);
        host[8 * i + 2] = fks_math::log(fks_math::dabs(y) + 1e-300);
        host[8 * i + 3] = fks_math::atan2(x, y);
        host[8 * i + 4] = fks_math::dsqrt(fks_math::dabs(y));
        host[8 * i + 5] = x / y;
        host[8 * i + 6] = fks_math::enforce_continuous_revolute_bounds(x / y); /* glibc fmod vs the kernel's wrap */
        host[8 * i + 7] = (x * y + x) * y - x * x;
    }
    DeviceBuffer<double> da, db, dout;
    if (upload(da, a.data(), n) != hipSuccess || upload(db, b.data(), n) != hipSuccess || dout.reserve(8 * n) != hipSuccess)
        return FKS_ERR_HIP;
    hipLaunchKernelGGL(fks_math_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                       static_cast<const double*>(da.get()), static_cast<const double*>(db.get()), dout.get(), n);
    if (hipMemcpy(dev.data(), dout.get(), 8 * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return FKS_ERR_HIP;
    uint64_t mism = 0;
    for (uint64_t i = 0; i < 8 * n; ++i)
        if (std::memcmp(&host[i], &dev[i], sizeof(double)) != 0) mism++;
    *out_mismatches = mism;
    return FKS_OK;
}

}  // extern "C"
