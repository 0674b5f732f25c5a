/* fks_launch.cpp — the launch decisions of fks_launch.h (no HIP runtime, no fks_context) */
#include "fks_launch.h"

#include <algorithm>

namespace fks_launch {

Family family_of(int32_t robot_type, bool lean) {
    return robot_type == FKS_ROBOT_SE2 ? SE2 : (robot_type == FKS_ROBOT_SE3 ? SE3 : (lean ? LINKED_LEAN : LINKED));
}

struct Row {
    KernelId id;
    const char* symbol;
};
static constexpr Row kRows[] = {
#define FKS_KERNEL(symbol, attributes, entry, flavour, form, budget, family) {{form, budget, family}, #symbol},
#define FKS_POLICY_KERNEL(symbol, attributes, entry, flavour, form, budget, family) {{form, budget, family}, #symbol},
#include "fks_kernel_list.h"
};
static_assert(sizeof(kRows) / sizeof(kRows[0]) == kKernelRows, "fks_kernel_list.h has kKernelRows rows");

/* the row of every identity, worked out at compile time so that a launch only indexes */
struct RowOf {
    int8_t row[FORM_COUNT][BUDGET_COUNT][FAMILY_COUNT];
};
static constexpr RowOf make_row_of() {
    RowOf t{};
    for (int f = 0; f < FORM_COUNT; ++f)
        for (int b = 0; b < BUDGET_COUNT; ++b)
            for (int m = 0; m < FAMILY_COUNT; ++m) t.row[f][b][m] = -1;
    for (int r = 0; r < kKernelRows; ++r) t.row[kRows[r].id.form][kRows[r].id.budget][kRows[r].id.family] = (int8_t)r;
    /* the one fallback: a lean robot runs the linked kernel where the list has no lean row */
    for (int f = 0; f < FORM_COUNT; ++f)
        for (int b = 0; b < BUDGET_COUNT; ++b)
            if (t.row[f][b][LINKED_LEAN] < 0) t.row[f][b][LINKED_LEAN] = t.row[f][b][LINKED];
    return t;
}
static constexpr RowOf kRowOf = make_row_of();
int kernel_row(const KernelId& id) {
    const bool known = (unsigned)id.form < FORM_COUNT && (unsigned)id.budget < BUDGET_COUNT && (unsigned)id.family < FAMILY_COUNT;
    return known ? kRowOf.row[id.form][id.budget][id.family] : -1;
}
const char* kernel_symbol(int row) { return row >= 0 && row < kKernelRows ? kRows[row].symbol : nullptr; }

/* resident waves per CU of a layout at the largest workgroup (<= wmax waves) whose blocks fit
 * the CU's LDS; *wpg and *bytes are that workgroup's also when nothing is resident */
static int resident_waves(const RobotShape& R, const Queries& q, const fksd::LdsLayout& l, uint32_t wmax, uint32_t* wpg,
                          size_t* bytes) {
    uint32_t w = wmax;
    size_t b = 0;
    for (;;) {
        b = ((size_t)l.shared_total + (size_t)w * l.total) * sizeof(double);
        if (b <= kCuLdsBytes || w == 1) break;
        w /= 2;
    }
    *wpg = w;
    *bytes = b;
    if (b > kCuLdsBytes) return 0;
    /* every kernel launched with this layout (plain, individual-Jacobian and traced simulation,
     * configuration check, kinematics) must hold that many groups: the smallest occupancy of
     * them all */
    const Family family = family_of(R.type, l.lean != 0);
    int n = 1 << 30;
    for (Form form : {PLAIN, INDIVIDUAL, TRACED, CHECK, KINEMATICS}) {
        const int nk = q.resident_blocks(KernelId{form, THROUGHPUT, family}, 64u * w, b);
        if (nk <= 0) return 0;
        n = std::min(n, nk);
    }
    return n * (int)w;
}

static fksd::LdsLayout lds_layout(const RobotShape& R, bool pair, bool lean) {
    return fksd::make_lds_layout(R.L, R.J, R.D, R.W, R.G, R.nrounds, pair, lean);
}

fks_status plan_layout(const LayoutInputs& in, const Queries& q, Layout* out, std::string* why) {
    const RobotShape& R = in.robot;
    Layout y;
    uint32_t wpg = 0;
    size_t bytes = 0;
    const bool linked_pairable = R.type == FKS_ROBOT_LINKED && R.J >= 1 && R.J <= 32;
    const int w0 = resident_waves(R, q, lds_layout(R, false, false), fksd::kWavesPerGroup, &wpg, &bytes);
    bool pair = false;
    if (linked_pairable && w0 > 0) {
        uint32_t w = 0;
        size_t b = 0;
        pair = resident_waves(R, q, lds_layout(R, true, false), fksd::kWavesPerGroup, &w, &b) >= w0;
    }
    int waves_per_cu = resident_waves(R, q, lds_layout(R, pair, false), fksd::kWavesPerGroup, &wpg, &bytes);
    const int standard_waves_per_cu = waves_per_cu;
    /* a linked robot whose LDS block caps the resident waves below the register limit may run
     * lean blocks (the skip-proof cache in scratch) in workgroups of up to 8 waves, if that
     * keeps more waves resident (cfg5's 14-dof arm: 12 -> 16 per CU) */
    bool lean = false;
    if (R.type == FKS_ROBOT_LINKED) {
        for (uint32_t wmax : {(uint32_t)fksd::kMaxWavesPerGroup, (uint32_t)fksd::kWavesPerGroup}) {
            uint32_t w = 0;
            size_t b = 0;
            const int n = resident_waves(R, q, lds_layout(R, false, true), wmax, &w, &b);
            if (n > waves_per_cu) {
                waves_per_cu = n;
                wpg = w;
                bytes = b;
                lean = true;
                pair = false;
            }
        }
    }
    if (waves_per_cu < 1) {
        *why = "robot too large: one wave's LDS block (" + std::to_string(bytes) + " bytes) does not fit a CU";
        return FKS_ERR_UNSUPPORTED;
    }
    uint32_t grid_groups = (uint32_t)(in.cus * (waves_per_cu / (int)wpg));
    y.scratch_per_wave = fksd::make_scratch_layout(3u * (uint32_t)R.P, R.D, R.P, R.G).total;
    /* the per-wave workspace grows with 3P x D (the stacked Jacobian) and the robot's
     * geometry count: for very large robots the persistent grid keeps only as many waves
     * as half the free HBM holds (the ticket queue hands out the work either way) */
    const size_t per_group = (size_t)wpg * y.scratch_per_wave * sizeof(double);
    const size_t max_groups = std::max<size_t>(1, ((size_t)in.free_hbm_bytes / 2) / std::max<size_t>(1, per_group));
    if ((size_t)grid_groups > max_groups) grid_groups = (uint32_t)max_groups;
    y.scratch_words = (uint64_t)grid_groups * wpg * y.scratch_per_wave;
    y.fk_pair = pair;
    y.lean = lean;
    y.standard_resident_waves = (uint32_t)(in.cus * std::max(0, standard_waves_per_cu));
    y.waves_per_cu = (uint32_t)waves_per_cu;
    y.waves_per_group = wpg;
    y.lds_bytes = bytes;
    y.grid_groups = grid_groups;
    y.grid_waves = grid_groups * wpg;
    const Family family = family_of(R.type, lean);
    /* the small-batch kernel on the same layout (not for lean blocks) */
    if (!lean) {
        const int nk = q.resident_blocks(KernelId{PLAIN, SMALL, family}, 64u * wpg, bytes);
        if (nk > 0) y.small_grid_waves = std::min<uint32_t>((uint32_t)(in.cus * nk) * wpg, y.grid_waves);
    }
    /* the cooperative kernel: one wave's block plus the mailbox per workgroup, its workgroup
     * size from its launch bound (a build's FKS_COOP_WAVES); each workgroup uses one wave's
     * workspace, so at most grid_waves of them */
    if (!lean && R.nrounds <= fksd::kCoopMaxRounds) {
        const fksd::LdsLayout l = lds_layout(R, pair, false);
        const size_t cb = ((size_t)l.shared_total + l.total + fksd::kCoopBoxDoubles) * sizeof(double);
        const KernelId coop{COOPERATIVE, THROUGHPUT, family};
        const int threads = cb <= kCuLdsBytes ? q.max_threads(coop) : 0;
        const int nk = threads >= kCoopMinThreads ? q.resident_blocks(coop, (uint32_t)threads, cb) : 0;
        if (nk > 0) {
            y.coop_waves = (uint32_t)threads / 64u;
            y.coop_lds_bytes = cb;
            y.coop_particles = std::min<uint32_t>((uint32_t)(in.cus * nk), y.grid_waves);
        }
    }
    *out = y;
    return FKS_OK;
}

/* whether a path, job or path-job batch may run the shaped batch kernels at all */
static bool batched_module_allowed(const Settings& s, const Request& rq) {
    return !rq.policy && rq.legs <= FKS_MAX_PATH_JOB_LEGS && s.bspec_enabled && s.specialize == FKS_SPECIALIZE_ON &&
           !s.individual_jacobians;
}
static bool cooperative_chosen(const Settings& s, const Request& rq) {
    return s.small_batch && s.cooperative && !s.individual_jacobians && !s.lean && rq.nseg == 1 && rq.n > 0 &&
           rq.n <= (uint64_t)s.coop_particles;
}

Module module_to_build(const Settings& s, const ModuleState& plain, const ModuleState& batched, const Request& rq) {
    switch (rq.kind) {
        case REQUEST_BATCH: return batched_module_allowed(s, rq) && batched.pending && !rq.small ? MODULE_BATCHED : MODULE_NONE;
        case REQUEST_CHECK: return plain.pending && rq.n > (uint64_t)s.grid_waves ? MODULE_PLAIN : MODULE_NONE;
        case REQUEST_TRACED: return MODULE_NONE;
        case REQUEST_PLAIN: break;
    }
    /* the plain throughput path alone runs the robot's shape-specialised kernel */
    return !cooperative_chosen(s, rq) && !rq.small && !s.individual_jacobians && plain.pending ? MODULE_PLAIN : MODULE_NONE;
}

Choice choose_kernel(const Settings& s, const ModuleState& plain, const ModuleState& batched, const Request& rq) {
    Choice c;
    const Family family = family_of(s.robot_type, s.lean);
    const Budget budget = rq.small ? SMALL : THROUGHPUT;
    auto generic = [&](int32_t kind, Form form, Budget b) {
        c.kind = kind;
        c.generic = KernelId{form, b, family};
    };
    auto shaped = [&](int32_t kind, Module m, ModuleFunction f) {
        c.kind = kind;
        c.module = m;
        c.function = f;
    };
    if (rq.kind == REQUEST_CHECK) {
        /* the shaped check runs whenever the module has it */
        generic(FKS_KERNEL_THROUGHPUT, CHECK, THROUGHPUT);
        if (plain.check_fn) shaped(FKS_KERNEL_SHAPED, MODULE_PLAIN, FUNCTION_CHECK);
    } else if (rq.kind == REQUEST_BATCH && rq.policy) {
        /* always the generic policy kernels, also when a batched shaped module exists */
        generic(rq.small ? FKS_KERNEL_POLICY_SMALL_BATCH : FKS_KERNEL_POLICY, POLICY, budget);
    } else if (rq.kind == REQUEST_BATCH) {
        /* the robot's batched module serves all three forms through its PATH && JOBS kernel when
         * the records fit its bound; otherwise the generic kernel of the batch's own form */
        static const int32_t kGeneric[3][2] = {{FKS_KERNEL_PATH, FKS_KERNEL_PATH_SMALL_BATCH},
                                               {FKS_KERNEL_JOBS, FKS_KERNEL_JOBS_SMALL_BATCH},
                                               {FKS_KERNEL_PATH_JOBS, FKS_KERNEL_PATH_JOBS_SMALL_BATCH}};
        generic(kGeneric[rq.form][rq.small ? 1 : 0], (Form)(PATH + rq.form), budget);
        const bool ready = rq.small ? (batched.fn && batched.small_fn && !s.lean) : batched.fn;
        if (batched_module_allowed(s, rq) && ready)
            shaped(rq.small ? FKS_KERNEL_SHAPED_PATH_JOBS_SMALL_BATCH : FKS_KERNEL_SHAPED_PATH_JOBS, MODULE_BATCHED,
                   rq.small ? FUNCTION_SMALL : FUNCTION_THROUGHPUT);
    } else if (rq.kind == REQUEST_TRACED) {
        generic(FKS_KERNEL_TRACED, TRACED, THROUGHPUT);
    } else if (cooperative_chosen(s, rq)) {
        generic(FKS_KERNEL_COOPERATIVE, COOPERATIVE, THROUGHPUT);
        c.cooperative = true;
    } else if (rq.small) {
        /* the shape's small-batch kernel once the robot's module is built */
        generic(FKS_KERNEL_SMALL_BATCH, PLAIN, SMALL);
        if (plain.fn && plain.small_fn) shaped(FKS_KERNEL_SHAPED_SMALL_BATCH, MODULE_PLAIN, FUNCTION_SMALL);
    } else if (s.individual_jacobians) {
        generic(FKS_KERNEL_INDIVIDUAL, INDIVIDUAL, THROUGHPUT);
    } else {
        generic(FKS_KERNEL_THROUGHPUT, PLAIN, THROUGHPUT);
        if (plain.fn) shaped(FKS_KERNEL_SHAPED, MODULE_PLAIN, FUNCTION_THROUGHPUT);
    }
    return c;
}

uint32_t groups_launched(uint64_t n, uint32_t waves_per_group, uint32_t resident_groups) {
    const uint64_t needed = (n + waves_per_group - 1) / waves_per_group;
    return (uint32_t)(needed < (uint64_t)resident_groups ? std::max<uint64_t>(needed, 1) : resident_groups);
}

Geometry launch_geometry(const Layout& l, uint64_t n, bool cooperative) {
    if (cooperative) return Geometry{(uint32_t)n, 64u * l.coop_waves, l.coop_lds_bytes};
    return Geometry{groups_launched(n, l.waves_per_group, l.grid_groups), 64u * l.waves_per_group, l.lds_bytes};
}

int throughput_register_budget(int waves_per_eu, int generic_registers) {
    return waves_per_eu > 0 ? (512 / waves_per_eu) & ~7 : generic_registers;
}

}  // namespace fks_launch
