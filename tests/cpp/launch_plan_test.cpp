/*
 * launch_plan_test.cpp — the launch decisions (csrc/fks_launch.h) without a GPU: the layout of a
 * robot against a fake occupancy query, the kernel and the module build of every kind of call,
 * the grid of a launch, the register gates, and the kernel list's identities.  Expected values
 * are worked out by hand; byte and word counts come from fksd::make_lds_layout /
 * make_scratch_layout.  Links fks_launch.cpp only.
 */
#include <cstdio>
#include <cstring>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "fks_launch.h"

using namespace fks_launch;

static int g_failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                  \
        }                                                                  \
    } while (0)

constexpr size_t kCu = 160 * 1024;
constexpr int kCus = 256;
constexpr uint64_t kPlentyHbm = 1ull << 40;

/* the fake runtime: answers from a function, remembers what it was asked */
struct Fake final : Queries {
    std::function<int(const KernelId&, uint32_t, size_t)> blocks;
    int bound = 512;
    mutable std::vector<KernelId> asked;
    mutable std::vector<uint32_t> asked_threads;
    int resident_blocks(const KernelId& id, uint32_t threads, size_t lds) const override {
        asked.push_back(id);
        asked_threads.push_back(threads);
        return blocks(id, threads, lds);
    }
    int max_threads(const KernelId&) const override { return bound; }
};
/* a CU: blocks that fit its LDS, at most `waves` resident waves (5 per SIMD: 20), 8 for the
 * two-waves-per-SIMD kernels */
static int cu_blocks(const KernelId& id, uint32_t threads, size_t lds, int waves = 20) {
    const int w = (id.budget == SMALL || id.form == COOPERATIVE) ? 8 : waves;
    return std::min((int)(kCu / lds), w / (int)(threads / 64));
}
static Fake cu_fake(int waves = 20) {
    Fake f;
    f.blocks = [waves](const KernelId& id, uint32_t t, size_t lds) { return cu_blocks(id, t, lds, waves); };
    return f;
}

static size_t block_bytes(const RobotShape& R, uint32_t waves, bool pair = false, bool lean = false) {
    const fksd::LdsLayout l = fksd::make_lds_layout(R.L, R.J, R.D, R.W, R.G, R.nrounds, pair, lean);
    return ((size_t)l.shared_total + (size_t)waves * l.total) * sizeof(double);
}
static uint64_t wave_words(const RobotShape& R) { return fksd::make_scratch_layout(3u * (uint32_t)R.P, R.D, R.P, R.G).total; }

static fks_status plan(const RobotShape& R, const Queries& q, Layout* y, std::string* why = nullptr, uint64_t hbm = kPlentyHbm) {
    std::string w;
    const fks_status st = plan_layout(LayoutInputs{R, kCus, hbm}, q, y, why ? why : &w);
    return st;
}

/* a free-flying body of L "links": no pairing, no lean block, so only the halving decides */
static RobotShape body(int L) { return RobotShape{FKS_ROBOT_SE3, L, 0, 6, 12, 1, 64, 1}; }
/* a 7-dof arm and a 14-dof dual arm */
static RobotShape arm(int32_t type = FKS_ROBOT_LINKED) { return RobotShape{type, 8, 7, 7, 7, 8, 512, 8}; }
static RobotShape dual_arm() { return RobotShape{FKS_ROBOT_LINKED, 17, 16, 14, 14, 17, 1088, 16}; }

static void test_workgroup_halving() {
    Layout y;
    /* fits at 4 waves; 5 blocks of every kernel */
    {
        const RobotShape R = body(1);
        EXPECT(block_bytes(R, 4) <= kCu);
        const Fake f = cu_fake();
        EXPECT(plan(R, f, &y) == FKS_OK);
        EXPECT(y.waves_per_group == 4 && y.lds_bytes == block_bytes(R, 4));
        EXPECT(y.waves_per_cu == 20 && y.standard_resident_waves == 256 * 20);
        EXPECT(y.grid_groups == 256 * 5 && y.grid_waves == 256 * 20);
        EXPECT(!y.fk_pair && !y.lean);
        EXPECT(y.scratch_per_wave == wave_words(R) && y.scratch_words == 5120ull * wave_words(R));
    }
    /* only at 2: one block per CU */
    {
        const RobotShape R = body(200);
        EXPECT(block_bytes(R, 4) > kCu && block_bytes(R, 2) <= kCu && 2 * block_bytes(R, 2) > kCu);
        EXPECT(plan(R, cu_fake(), &y) == FKS_OK);
        EXPECT(y.waves_per_group == 2 && y.lds_bytes == block_bytes(R, 2));
        EXPECT(y.waves_per_cu == 2 && y.grid_groups == 256 && y.grid_waves == 512);
    }
    /* only at 1 */
    {
        const RobotShape R = body(400);
        EXPECT(block_bytes(R, 2) > kCu && block_bytes(R, 1) <= kCu);
        EXPECT(plan(R, cu_fake(), &y) == FKS_OK);
        EXPECT(y.waves_per_group == 1 && y.lds_bytes == block_bytes(R, 1));
        EXPECT(y.waves_per_cu == 1 && y.grid_groups == 256 && y.grid_waves == 256);
    }
}

static void test_refusals() {
    Layout y;
    y.grid_waves = 77; /* untouched by a refusal */
    std::string why;
    /* one wave's block does not fit */
    for (int32_t type : {FKS_ROBOT_SE3, FKS_ROBOT_LINKED}) {
        RobotShape R = body(600);
        R.type = type;
        R.J = type == FKS_ROBOT_LINKED ? 1 : 0;
        EXPECT(block_bytes(R, 1) > kCu && block_bytes(R, 1, false, true) > kCu);
        EXPECT(plan(R, cu_fake(), &y, &why) == FKS_ERR_UNSUPPORTED);
        EXPECT(why == "robot too large: one wave's LDS block (" + std::to_string(block_bytes(R, 1)) + " bytes) does not fit a CU");
    }
    /* the occupancy query fails: the same refusal, with the block that was asked about */
    {
        Fake f;
        f.blocks = [](const KernelId&, uint32_t, size_t) { return 0; };
        const RobotShape R = body(1);
        EXPECT(plan(R, f, &y, &why) == FKS_ERR_UNSUPPORTED);
        EXPECT(why == "robot too large: one wave's LDS block (" + std::to_string(block_bytes(R, 4)) + " bytes) does not fit a CU");
    }
    EXPECT(y.grid_waves == 77);
}

static void test_minimum_over_kernels() {
    const RobotShape R = body(1);
    for (Form low : {PLAIN, INDIVIDUAL, TRACED, CHECK, KINEMATICS}) {
        Fake f;
        f.blocks = [low](const KernelId& id, uint32_t, size_t) { return id.form == low && id.budget == THROUGHPUT ? 3 : 5; };
        Layout y;
        EXPECT(plan(R, f, &y) == FKS_OK);
        EXPECT(y.waves_per_cu == 12 && y.grid_groups == 256 * 3 && y.grid_waves == 256 * 12);
    }
    /* a kernel that is not launched with the layout is not asked about */
    Fake f;
    f.blocks = [](const KernelId& id, uint32_t, size_t) { return id.form >= PATH ? 1 : 5; };
    Layout y;
    EXPECT(plan(R, f, &y) == FKS_OK && y.waves_per_cu == 20);
    for (const KernelId& id : f.asked) EXPECT(id.form < PATH && id.family == SE3);
}

/* the fake of the pairing and lean cases: blocks by the LDS bytes asked about */
static Fake by_bytes(const RobotShape& R, int plain4, int pair4, int lean8, int lean4, int small = 2) {
    const size_t bp = block_bytes(R, 4), bq = block_bytes(R, 4, true), l8 = block_bytes(R, 8, false, true),
                 l4 = block_bytes(R, 4, false, true);
    Fake f;
    f.blocks = [=](const KernelId& id, uint32_t threads, size_t lds) {
        if (id.budget == SMALL) return small;
        if (id.form == COOPERATIVE) return 1;
        if (lds == l8 && threads == 512) return lean8;
        if (lds == l4 && threads == 256) return lean4;
        if (lds == bq) return pair4;
        return lds == bp ? plain4 : -1000;
    };
    return f;
}

static void test_pairing() {
    const RobotShape R = arm();
    EXPECT(block_bytes(R, 4, true) > block_bytes(R, 4) && block_bytes(R, 8, false, true) <= kCu);
    Layout y;
    /* taken at equal occupancy */
    EXPECT(plan(R, by_bytes(R, 5, 5, 2, 5), &y) == FKS_OK);
    EXPECT(y.fk_pair && !y.lean && y.lds_bytes == block_bytes(R, 4, true) && y.waves_per_cu == 20);
    /* refused at lower */
    EXPECT(plan(R, by_bytes(R, 5, 4, 2, 5), &y) == FKS_OK);
    EXPECT(!y.fk_pair && !y.lean && y.lds_bytes == block_bytes(R, 4) && y.waves_per_cu == 20);
    /* 1 <= J <= 32 */
    const RobotShape j32{FKS_ROBOT_LINKED, 33, 32, 32, 32, 33, 528, 9}, j33{FKS_ROBOT_LINKED, 34, 33, 32, 32, 34, 544, 9},
        j0{FKS_ROBOT_LINKED, 1, 0, 1, 1, 1, 64, 1};
    EXPECT(plan(j32, by_bytes(j32, 5, 5, 2, 5), &y) == FKS_OK && y.fk_pair && y.lds_bytes == block_bytes(j32, 4, true));
    EXPECT(plan(j33, by_bytes(j33, 5, 5, 2, 5), &y) == FKS_OK && !y.fk_pair && y.lds_bytes == block_bytes(j33, 4));
    EXPECT(plan(j0, by_bytes(j0, 5, 5, 2, 5), &y) == FKS_OK && !y.fk_pair && y.lds_bytes == block_bytes(j0, 4));
    /* SE(2) and SE(3) never */
    for (int32_t type : {FKS_ROBOT_SE2, FKS_ROBOT_SE3}) {
        EXPECT(plan(arm(type), cu_fake(), &y) == FKS_OK);
        EXPECT(!y.fk_pair && y.lds_bytes == block_bytes(arm(type), 4) && y.waves_per_cu == 20);
    }
}

static void test_lean() {
    const RobotShape R = arm();
    Layout y;
    /* only at strictly more waves: 12 standard, the lean blocks 8 and 12 */
    EXPECT(plan(R, by_bytes(R, 3, 2, 1, 3), &y) == FKS_OK);
    EXPECT(!y.lean && !y.fk_pair && y.waves_per_cu == 12 && y.waves_per_group == 4 && y.lds_bytes == block_bytes(R, 4));
    EXPECT(y.small_grid_waves == 256 * 2 * 4);
    /* the 8-wave attempt before the 4-wave one: both give 16, the first one stays */
    {
        const Fake f = by_bytes(R, 3, 2, 2, 4);
        EXPECT(plan(R, f, &y) == FKS_OK);
        EXPECT(y.lean && y.waves_per_cu == 16 && y.waves_per_group == 8 && y.lds_bytes == block_bytes(R, 8, false, true));
        EXPECT(y.grid_groups == 256 * 2 && y.grid_waves == 256 * 16);
        EXPECT(y.standard_resident_waves == 256 * 12); /* still the non-lean figure */
        EXPECT(y.small_grid_waves == 0 && y.coop_particles == 0 && y.coop_waves == 0 && y.coop_lds_bytes == 0);
        for (const KernelId& id : f.asked) EXPECT(id.budget == THROUGHPUT && id.form != COOPERATIVE);
    }
    /* the 4-wave one when only it gains */
    EXPECT(plan(R, by_bytes(R, 3, 2, 1, 4), &y) == FKS_OK);
    EXPECT(y.lean && y.waves_per_cu == 16 && y.waves_per_group == 4 && y.lds_bytes == block_bytes(R, 4, false, true));
    /* lean clears fk_pair */
    EXPECT(plan(R, by_bytes(R, 3, 3, 2, 3), &y) == FKS_OK);
    EXPECT(y.lean && !y.fk_pair && y.waves_per_cu == 16 && y.standard_resident_waves == 256 * 12);
    /* ... which it had: the same robot without the lean gain */
    EXPECT(plan(R, by_bytes(R, 3, 3, 1, 3), &y) == FKS_OK);
    EXPECT(!y.lean && y.fk_pair);
    /* the dual arm on a CU of 20 waves: three standard blocks of 4 fit the LDS, two lean ones of 8 (12 -> 16) */
    {
        const RobotShape D = dual_arm();
        EXPECT(kCu / block_bytes(D, 4) == 3 && kCu / block_bytes(D, 8, false, true) == 2);
        EXPECT(plan(D, cu_fake(), &y) == FKS_OK);
        EXPECT(y.lean && !y.fk_pair && y.waves_per_group == 8 && y.waves_per_cu == 16 && y.lds_bytes == block_bytes(D, 8, false, true));
        EXPECT(y.standard_resident_waves == 256 * 12 && y.grid_waves == 256 * 16);
    }
    /* never for SE(2) / SE(3): an LDS-bound CU (64 waves of registers) where a linked robot goes lean */
    EXPECT(plan(R, cu_fake(64), &y) == FKS_OK && y.lean && y.waves_per_group == 8);
    for (int32_t type : {FKS_ROBOT_SE2, FKS_ROBOT_SE3}) {
        const Fake f = cu_fake(64);
        EXPECT(plan(arm(type), f, &y) == FKS_OK);
        EXPECT(!y.lean && y.waves_per_group == 4 && y.lds_bytes == block_bytes(arm(type), 4));
        for (const KernelId& id : f.asked) EXPECT(id.family == (type == FKS_ROBOT_SE2 ? SE2 : SE3));
    }
}

static void test_hbm_cap() {
    const RobotShape R = body(1);
    const uint64_t spw = wave_words(R), per_group = 4 * spw * sizeof(double);
    struct Case {
        uint64_t free_bytes;
        uint32_t groups;
    };
    /* the uncapped grid: 256 x 5 groups */
    const Case cases[] = {{2 * per_group * 1279, 1279}, {2 * per_group * 1279 + 2 * per_group - 1, 1279}, {2 * per_group * 1280, 1280},
                          {2 * per_group * 1281, 1280}, {2 * per_group * 100, 100},  {0, 1},
                          {per_group, 1}};
    for (const Case& c : cases) {
        Layout y;
        EXPECT(plan(R, cu_fake(), &y, nullptr, c.free_bytes) == FKS_OK);
        EXPECT(y.grid_groups == c.groups && y.grid_waves == 4 * c.groups);
        EXPECT(y.scratch_per_wave == spw && y.scratch_words == (uint64_t)c.groups * 4 * spw);
        EXPECT(y.waves_per_cu == 20 && y.standard_resident_waves == 5120); /* what the CU holds, not the cap */
    }
}

static void test_small_batch() {
    const RobotShape R = body(1);
    Layout y;
    auto small_blocks = [](int small) {
        Fake f;
        f.blocks = [small](const KernelId& id, uint32_t, size_t) { return id.budget == SMALL ? small : 5; };
        return f;
    };
    /* min(cus x nk x wpg, grid_waves) */
    EXPECT(plan(R, small_blocks(3), &y) == FKS_OK && y.small_grid_waves == 256 * 3 * 4);
    EXPECT(plan(R, small_blocks(7), &y) == FKS_OK && y.small_grid_waves == 5120);
    const uint64_t per_group = 4 * wave_words(R) * sizeof(double);
    EXPECT(plan(R, small_blocks(3), &y, nullptr, 2 * per_group * 100) == FKS_OK && y.small_grid_waves == 400);
    /* the small-batch kernel is asked about at the layout's workgroup and block */
    {
        const Fake f = small_blocks(3);
        EXPECT(plan(R, f, &y) == FKS_OK);
        bool asked = false;
        for (size_t k = 0; k < f.asked.size(); ++k)
            if (f.asked[k].budget == SMALL) asked = f.asked[k].form == PLAIN && f.asked_threads[k] == 256;
        EXPECT(asked);
    }
    /* 0 when the query fails; 0 when lean (test_lean) */
    EXPECT(plan(R, small_blocks(0), &y) == FKS_OK && y.small_grid_waves == 0 && y.grid_waves == 5120);
}

static void test_cooperative() {
    const RobotShape R = arm();
    const fksd::LdsLayout paired = fksd::make_lds_layout(R.L, R.J, R.D, R.W, R.G, R.nrounds, true);
    const size_t coop_bytes = ((size_t)paired.shared_total + paired.total + fksd::kCoopBoxDoubles) * sizeof(double);
    auto coop_blocks = [](int coop, int bound) {
        Fake f;
        f.bound = bound;
        f.blocks = [coop](const KernelId& id, uint32_t threads, size_t lds) {
            return id.form == COOPERATIVE ? coop : cu_blocks(id, threads, lds);
        };
        return f;
    };
    Layout y;
    /* min(cus x nk, grid_waves), the waves from the launch bound, one paired block plus the mailbox */
    {
        const Fake f = coop_blocks(2, 512);
        EXPECT(plan(R, f, &y) == FKS_OK && y.fk_pair);
        EXPECT(y.coop_particles == 512 && y.coop_waves == 8 && y.coop_lds_bytes == coop_bytes);
        bool asked = false;
        for (size_t k = 0; k < f.asked.size(); ++k)
            if (f.asked[k].form == COOPERATIVE) asked = f.asked_threads[k] == 512 && f.asked[k].family == LINKED;
        EXPECT(asked);
    }
    EXPECT(plan(R, coop_blocks(2, 256), &y) == FKS_OK && y.coop_particles == 512 && y.coop_waves == 4);
    EXPECT(plan(R, coop_blocks(2, 128), &y) == FKS_OK && y.coop_particles == 512 && y.coop_waves == 2);
    const uint64_t per_group = 4 * wave_words(R) * sizeof(double);
    EXPECT(plan(R, coop_blocks(2, 512), &y, nullptr, 2 * per_group * 100) == FKS_OK && y.coop_particles == 400);
    /* a launch bound below 128 */
    EXPECT(plan(R, coop_blocks(2, 64), &y) == FKS_OK);
    EXPECT(y.coop_particles == 0 && y.coop_waves == 0 && y.coop_lds_bytes == 0);
    EXPECT(plan(R, coop_blocks(2, 0), &y) == FKS_OK && y.coop_particles == 0); /* the bound's query failed */
    EXPECT(plan(R, coop_blocks(0, 512), &y) == FKS_OK && y.coop_particles == 0 && y.coop_waves == 0 && y.coop_lds_bytes == 0);
    /* 16 rounds are allowed, 17 not */
    RobotShape r16 = R, r17 = R;
    r16.nrounds = 16;
    r17.nrounds = 17;
    EXPECT(plan(r16, by_bytes(r16, 5, 5, 2, 5), &y) == FKS_OK && y.coop_particles == 256 && y.coop_waves == 8);
    EXPECT(plan(r17, by_bytes(r17, 5, 5, 2, 5), &y) == FKS_OK && y.coop_particles == 0 && y.coop_waves == 0);
    /* a block that fits a CU alone and not with the mailbox */
    {
        RobotShape B = body(400);
        bool found = false;
        for (B.W = 1; B.W < 2000 && !found; ++B.W) {
            const size_t one = block_bytes(B, 1);
            found = one <= kCu && one + fksd::kCoopBoxDoubles * sizeof(double) > kCu;
            if (found) break;
        }
        EXPECT(found);
        EXPECT(plan(B, coop_blocks(1, 512), &y) == FKS_OK && y.waves_per_group == 1 && y.grid_waves == 256);
        EXPECT(y.coop_particles == 0 && y.coop_waves == 0 && y.coop_lds_bytes == 0);
        B.W -= 8; /* with room for the mailbox */
        EXPECT(block_bytes(B, 1) + fksd::kCoopBoxDoubles * sizeof(double) <= kCu);
        EXPECT(plan(B, coop_blocks(1, 512), &y) == FKS_OK && y.coop_particles == 256);
    }
    /* lean: test_lean */
}

/* ---- the kernel of a call ---- */
static Settings settings() {
    Settings s;
    s.robot_type = FKS_ROBOT_LINKED;
    s.coop_particles = 256;
    s.grid_waves = 5120;
    return s;
}
static ModuleState module(bool fn, bool small_fn = false, bool check_fn = false, bool pending = false) {
    ModuleState m;
    m.fn = fn;
    m.small_fn = small_fn;
    m.check_fn = check_fn;
    m.pending = pending;
    return m;
}
static const ModuleState kAbsent = module(false), kPending = module(false, false, false, true), kBuilt = module(true, true, true),
                         kBuiltNoSmall = module(true, false, true);
static Request request(RequestKind kind, uint64_t n, bool small = false, uint32_t nseg = 1) {
    Request r;
    r.kind = kind;
    r.n = n;
    r.small = small;
    r.nseg = nseg;
    return r;
}
static Request batch(fks_batch::Form form, bool small, uint64_t legs = 3, bool policy = false) {
    Request r = request(REQUEST_BATCH, 64, small);
    r.form = form;
    r.legs = legs;
    r.policy = policy;
    return r;
}
static const char* symbol(const Choice& c) { return kernel_symbol(kernel_row(c.generic)); }
static bool runs_generic(const Choice& c, int32_t kind, const char* name) {
    return c.kind == kind && c.module == MODULE_NONE && c.function == FUNCTION_NONE && !c.cooperative && symbol(c) &&
           std::strcmp(symbol(c), name) == 0;
}
static bool runs_shaped(const Choice& c, int32_t kind, Module m, ModuleFunction f) {
    return c.kind == kind && c.module == m && c.function == f && !c.cooperative;
}

static void test_plain_calls() {
    const Settings s = settings();
    Settings lean = s;
    lean.lean = true;
    /* traced: whole, generic, builds nothing */
    const Request traced = request(REQUEST_TRACED, 16, true);
    EXPECT(module_to_build(s, kPending, kPending, traced) == MODULE_NONE);
    EXPECT(runs_generic(choose_kernel(s, kBuilt, kBuilt, traced), FKS_KERNEL_TRACED, "fks_simulate_linked_traced"));
    EXPECT(runs_generic(choose_kernel(lean, kBuilt, kBuilt, traced), FKS_KERNEL_TRACED, "fks_simulate_linked_lean_traced"));
    /* cooperative: its seven conditions together ... */
    Settings coop = s;
    coop.cooperative = true;
    const Request few = request(REQUEST_PLAIN, 16, true);
    {
        const Choice c = choose_kernel(coop, kBuilt, kBuilt, few);
        EXPECT(c.kind == FKS_KERNEL_COOPERATIVE && c.cooperative && c.module == MODULE_NONE);
        EXPECT(std::strcmp(symbol(c), "fks_simulate_linked_coop") == 0);
        EXPECT(module_to_build(coop, kPending, kPending, request(REQUEST_PLAIN, 16, false)) == MODULE_NONE);
        EXPECT(choose_kernel(coop, kBuilt, kBuilt, request(REQUEST_PLAIN, 256, true)).cooperative); /* n at coop_particles */
    }
    /* ... and each one failing alone */
    {
        Settings a = coop, b = coop, c = coop, d = coop;
        a.small_batch = false;
        b.cooperative = false;
        c.individual_jacobians = true;
        d.lean = true;
        for (const Settings& x : {a, b, c, d}) {
            const Choice ch = choose_kernel(x, kAbsent, kAbsent, few);
            EXPECT(!ch.cooperative && ch.kind == FKS_KERNEL_SMALL_BATCH);
        }
        for (const Request& r : {request(REQUEST_PLAIN, 16, true, 2), request(REQUEST_PLAIN, 0, true), request(REQUEST_PLAIN, 257, true)}) {
            const Choice ch = choose_kernel(coop, kAbsent, kAbsent, r);
            EXPECT(!ch.cooperative && ch.kind == FKS_KERNEL_SMALL_BATCH);
        }
        /* a call that would have been cooperative builds the pending module once it is not */
        EXPECT(module_to_build(coop, kPending, kPending, request(REQUEST_PLAIN, 257, false)) == MODULE_PLAIN);
    }
    /* small: the module's small function when it has both, and never a build */
    const Request small = request(REQUEST_PLAIN, 100, true);
    EXPECT(module_to_build(s, kPending, kPending, small) == MODULE_NONE);
    EXPECT(runs_shaped(choose_kernel(s, kBuilt, kAbsent, small), FKS_KERNEL_SHAPED_SMALL_BATCH, MODULE_PLAIN, FUNCTION_SMALL));
    EXPECT(runs_generic(choose_kernel(s, kBuiltNoSmall, kBuilt, small), FKS_KERNEL_SMALL_BATCH, "fks_simulate_linked_small"));
    EXPECT(runs_generic(choose_kernel(s, module(false, true), kBuilt, small), FKS_KERNEL_SMALL_BATCH, "fks_simulate_linked_small"));
    EXPECT(runs_generic(choose_kernel(s, kPending, kBuilt, small), FKS_KERNEL_SMALL_BATCH, "fks_simulate_linked_small"));
    /* individual Jacobians: generic, builds nothing */
    Settings indiv = s;
    indiv.individual_jacobians = true;
    const Request many = request(REQUEST_PLAIN, 100000, false, 15);
    EXPECT(module_to_build(indiv, kPending, kPending, many) == MODULE_NONE);
    EXPECT(runs_generic(choose_kernel(indiv, kBuilt, kBuilt, many), FKS_KERNEL_INDIVIDUAL, "fks_simulate_linked_indiv"));
    Settings lean_indiv = indiv;
    lean_indiv.lean = true;
    EXPECT(runs_generic(choose_kernel(lean_indiv, kBuilt, kBuilt, many), FKS_KERNEL_INDIVIDUAL, "fks_simulate_linked_lean_indiv"));
    /* throughput: the module absent, present, pending (built first) */
    EXPECT(module_to_build(s, kAbsent, kPending, many) == MODULE_NONE);
    EXPECT(runs_generic(choose_kernel(s, kAbsent, kBuilt, many), FKS_KERNEL_THROUGHPUT, "fks_simulate_linked"));
    EXPECT(runs_generic(choose_kernel(lean, kAbsent, kBuilt, many), FKS_KERNEL_THROUGHPUT, "fks_simulate_linked_lean"));
    EXPECT(module_to_build(s, kBuilt, kPending, many) == MODULE_NONE);
    EXPECT(runs_shaped(choose_kernel(s, kBuilt, kAbsent, many), FKS_KERNEL_SHAPED, MODULE_PLAIN, FUNCTION_THROUGHPUT));
    EXPECT(module_to_build(s, kPending, kAbsent, many) == MODULE_PLAIN);
    Settings se3 = s;
    se3.robot_type = FKS_ROBOT_SE3;
    EXPECT(runs_generic(choose_kernel(se3, kAbsent, kAbsent, many), FKS_KERNEL_THROUGHPUT, "fks_simulate_se3"));
}

static void test_checks() {
    const Settings s = settings();
    /* the module is built only for more configurations than the grid has waves ... */
    EXPECT(module_to_build(s, kPending, kPending, request(REQUEST_CHECK, 5120)) == MODULE_NONE);
    EXPECT(module_to_build(s, kPending, kPending, request(REQUEST_CHECK, 5121)) == MODULE_PLAIN);
    EXPECT(module_to_build(s, kAbsent, kPending, request(REQUEST_CHECK, 5121)) == MODULE_NONE);
    EXPECT(module_to_build(s, kBuilt, kPending, request(REQUEST_CHECK, 5121)) == MODULE_NONE);
    /* ... and its check runs whenever it is there */
    for (uint64_t n : {1ull, 5120ull, 5121ull}) {
        EXPECT(runs_generic(choose_kernel(s, kAbsent, kBuilt, request(REQUEST_CHECK, n)), FKS_KERNEL_THROUGHPUT, "fks_check_configs_linked"));
        EXPECT(runs_generic(choose_kernel(s, kPending, kBuilt, request(REQUEST_CHECK, n)), FKS_KERNEL_THROUGHPUT, "fks_check_configs_linked"));
        EXPECT(runs_generic(choose_kernel(s, module(true, true, false), kBuilt, request(REQUEST_CHECK, n)), FKS_KERNEL_THROUGHPUT,
                           "fks_check_configs_linked"));
        EXPECT(runs_shaped(choose_kernel(s, kBuilt, kAbsent, request(REQUEST_CHECK, n)), FKS_KERNEL_SHAPED, MODULE_PLAIN, FUNCTION_CHECK));
    }
    Settings lean = s;
    lean.lean = true;
    EXPECT(runs_generic(choose_kernel(lean, kAbsent, kAbsent, request(REQUEST_CHECK, 9)), FKS_KERNEL_THROUGHPUT, "fks_check_configs_linked"));
}

static void test_batches() {
    static const char* const kNames[3][2] = {{"fks_simulate_linked_path", "fks_simulate_linked_path_small"},
                                             {"fks_simulate_linked_jobs", "fks_simulate_linked_jobs_small"},
                                             {"fks_simulate_linked_path_jobs", "fks_simulate_linked_path_jobs_small"}};
    static const char* const kLeanNames[3] = {"fks_simulate_linked_lean_path", "fks_simulate_linked_lean_jobs",
                                              "fks_simulate_linked_lean_path_jobs"};
    static const int32_t kKinds[3][2] = {{FKS_KERNEL_PATH, FKS_KERNEL_PATH_SMALL_BATCH},
                                         {FKS_KERNEL_JOBS, FKS_KERNEL_JOBS_SMALL_BATCH},
                                         {FKS_KERNEL_PATH_JOBS, FKS_KERNEL_PATH_JOBS_SMALL_BATCH}};
    Settings on = settings();
    on.bspec_enabled = true;
    Settings off = on, indiv = on, no_proofs = on, spec_off = on, lean = on;
    off.bspec_enabled = false;
    indiv.individual_jacobians = true;
    no_proofs.specialize = FKS_SPECIALIZE_NO_PROOFS;
    spec_off.specialize = FKS_SPECIALIZE_OFF;
    lean.lean = true;
    for (int form = 0; form < 3; ++form)
        for (int small = 0; small < 2; ++small) {
            const Request rq = batch((fks_batch::Form)form, small != 0);
            const int32_t generic_kind = kKinds[form][small];
            const char* generic_name = kNames[form][small];
            const int32_t shaped_kind = small ? FKS_KERNEL_SHAPED_PATH_JOBS_SMALL_BATCH : FKS_KERNEL_SHAPED_PATH_JOBS;
            const ModuleFunction shaped_fn = small ? FUNCTION_SMALL : FUNCTION_THROUGHPUT;
            /* the batched module off, individual Jacobians, a mode that is not ON: generic, no build */
            for (const Settings& x : {off, indiv, no_proofs, spec_off}) {
                EXPECT(module_to_build(x, kPending, kPending, rq) == MODULE_NONE);
                EXPECT(runs_generic(choose_kernel(x, kBuilt, kBuilt, rq), generic_kind, generic_name));
            }
            /* pending: built first, unless the batch is small */
            EXPECT(module_to_build(on, kPending, kPending, rq) == (small ? MODULE_NONE : MODULE_BATCHED));
            EXPECT(runs_generic(choose_kernel(on, kBuilt, kPending, rq), generic_kind, generic_name));
            EXPECT(module_to_build(on, kPending, kAbsent, rq) == MODULE_NONE);
            EXPECT(runs_generic(choose_kernel(on, kBuilt, kAbsent, rq), generic_kind, generic_name)); /* its build failed */
            /* built */
            EXPECT(module_to_build(on, kPending, kBuilt, rq) == MODULE_NONE);
            EXPECT(runs_shaped(choose_kernel(on, kAbsent, kBuilt, rq), shaped_kind, MODULE_BATCHED, shaped_fn));
            /* built without its small function */
            if (small) EXPECT(runs_generic(choose_kernel(on, kBuilt, kBuiltNoSmall, rq), generic_kind, generic_name));
            else EXPECT(runs_shaped(choose_kernel(on, kBuilt, kBuiltNoSmall, rq), shaped_kind, MODULE_BATCHED, shaped_fn));
            /* lean: no shaped small kernel; the generic kernels are the lean ones where the list has them */
            if (small) EXPECT(runs_generic(choose_kernel(lean, kBuilt, kBuilt, rq), generic_kind, generic_name));
            else EXPECT(runs_shaped(choose_kernel(lean, kBuilt, kBuilt, rq), shaped_kind, MODULE_BATCHED, shaped_fn));
            if (!small) EXPECT(runs_generic(choose_kernel(lean, kBuilt, kAbsent, rq), generic_kind, kLeanNames[form]));
            /* legs at the bound and one above it */
            const Request at = batch((fks_batch::Form)form, small != 0, FKS_MAX_PATH_JOB_LEGS),
                          above = batch((fks_batch::Form)form, small != 0, (uint64_t)FKS_MAX_PATH_JOB_LEGS + 1);
            EXPECT(module_to_build(on, kAbsent, kPending, at) == (small ? MODULE_NONE : MODULE_BATCHED));
            EXPECT(runs_shaped(choose_kernel(on, kAbsent, kBuilt, at), shaped_kind, MODULE_BATCHED, shaped_fn));
            EXPECT(module_to_build(on, kAbsent, kPending, above) == MODULE_NONE);
            EXPECT(runs_generic(choose_kernel(on, kAbsent, kBuilt, above), generic_kind, generic_name));
        }
    /* a policy roll-out: never shaped, never builds */
    for (int small = 0; small < 2; ++small) {
        const Request rq = batch(fks_batch::PATH, small != 0, 3, true);
        EXPECT(module_to_build(on, kPending, kPending, rq) == MODULE_NONE);
        EXPECT(runs_generic(choose_kernel(on, kBuilt, kBuilt, rq), small ? FKS_KERNEL_POLICY_SMALL_BATCH : FKS_KERNEL_POLICY,
                           small ? "fks_simulate_linked_policy_small" : "fks_simulate_linked_policy"));
    }
    EXPECT(runs_generic(choose_kernel(lean, kBuilt, kBuilt, batch(fks_batch::PATH, false, 3, true)), FKS_KERNEL_POLICY,
                       "fks_simulate_linked_lean_policy"));
}

static void test_grid() {
    /* 1280 resident groups of 4 waves */
    EXPECT(groups_launched(0, 4, 1280) == 1); /* a simulation of no particle still launches */
    EXPECT(groups_launched(1, 4, 1280) == 1);
    EXPECT(groups_launched(4, 4, 1280) == 1);
    EXPECT(groups_launched(5, 4, 1280) == 2);
    EXPECT(groups_launched(5116, 4, 1280) == 1279);
    EXPECT(groups_launched(5117, 4, 1280) == 1280);
    EXPECT(groups_launched(5120, 4, 1280) == 1280);
    EXPECT(groups_launched(5121, 4, 1280) == 1280);
    EXPECT(groups_launched(0xffffffffull, 4, 1280) == 1280);
    EXPECT(groups_launched(0xffffffffull, 1, 0xffffffffu) == 0xffffffffu);
    EXPECT(groups_launched(0xffffffffull, 8, 0xffffffffu) == 0x20000000u);
    Layout y;
    y.waves_per_group = 8;
    y.grid_groups = 512;
    y.lds_bytes = 81504;
    y.coop_waves = 4;
    y.coop_lds_bytes = 7000;
    const Geometry g = launch_geometry(y, 100), all = launch_geometry(y, 1u << 20), none = launch_geometry(y, 0),
                   coop = launch_geometry(y, 100, true);
    EXPECT(g.blocks == 13 && g.threads == 512 && g.lds_bytes == 81504);
    EXPECT(all.blocks == 512 && none.blocks == 1);
    EXPECT(coop.blocks == 100 && coop.threads == 256 && coop.lds_bytes == 7000);
}

static void test_register_gates() {
    EXPECT(throughput_register_budget(5, 64) == 96); /* 512 / 5 = 102, in granules of 8 */
    EXPECT(throughput_register_budget(4, 64) == 128);
    EXPECT(throughput_register_budget(3, 64) == 168);
    EXPECT(throughput_register_budget(1, 64) == 512);
    EXPECT(throughput_register_budget(0, 77) == 77); /* the generic kernel's own count */
    EXPECT(kSmallRegisterBound == 256);
}

static void test_kernel_list() {
    EXPECT(family_of(FKS_ROBOT_LINKED, false) == LINKED && family_of(FKS_ROBOT_LINKED, true) == LINKED_LEAN);
    EXPECT(family_of(FKS_ROBOT_SE2, false) == SE2 && family_of(FKS_ROBOT_SE2, true) == SE2);
    EXPECT(family_of(FKS_ROBOT_SE3, false) == SE3 && family_of(FKS_ROBOT_SE3, true) == SE3);
    struct Named {
        Form form;
        Budget budget;
        const char* names[4]; /* linked, linked lean, SE(2), SE(3) */
    };
    /* every kernel by form, budget and family, the lean robot's fallbacks written out */
    static const Named kAll[] = {
        {PLAIN, THROUGHPUT, {"fks_simulate_linked", "fks_simulate_linked_lean", "fks_simulate_se2", "fks_simulate_se3"}},
        {PLAIN, SMALL, {"fks_simulate_linked_small", "fks_simulate_linked_small", "fks_simulate_se2_small", "fks_simulate_se3_small"}},
        {INDIVIDUAL, THROUGHPUT,
         {"fks_simulate_linked_indiv", "fks_simulate_linked_lean_indiv", "fks_simulate_se2_indiv", "fks_simulate_se3_indiv"}},
        {TRACED, THROUGHPUT,
         {"fks_simulate_linked_traced", "fks_simulate_linked_lean_traced", "fks_simulate_se2_traced", "fks_simulate_se3_traced"}},
        {COOPERATIVE, THROUGHPUT, {"fks_simulate_linked_coop", "fks_simulate_linked_coop", "fks_simulate_se2_coop", "fks_simulate_se3_coop"}},
        {CHECK, THROUGHPUT, {"fks_check_configs_linked", "fks_check_configs_linked", "fks_check_configs_se2", "fks_check_configs_se3"}},
        {KINEMATICS, THROUGHPUT, {"fks_kinematics_linked", "fks_kinematics_linked", "fks_kinematics_se2", "fks_kinematics_se3"}},
        {PATH, THROUGHPUT, {"fks_simulate_linked_path", "fks_simulate_linked_lean_path", "fks_simulate_se2_path", "fks_simulate_se3_path"}},
        {PATH, SMALL,
         {"fks_simulate_linked_path_small", "fks_simulate_linked_path_small", "fks_simulate_se2_path_small", "fks_simulate_se3_path_small"}},
        {JOBS, THROUGHPUT, {"fks_simulate_linked_jobs", "fks_simulate_linked_lean_jobs", "fks_simulate_se2_jobs", "fks_simulate_se3_jobs"}},
        {JOBS, SMALL,
         {"fks_simulate_linked_jobs_small", "fks_simulate_linked_jobs_small", "fks_simulate_se2_jobs_small", "fks_simulate_se3_jobs_small"}},
        {PATH_JOBS, THROUGHPUT,
         {"fks_simulate_linked_path_jobs", "fks_simulate_linked_lean_path_jobs", "fks_simulate_se2_path_jobs", "fks_simulate_se3_path_jobs"}},
        {PATH_JOBS, SMALL,
         {"fks_simulate_linked_path_jobs_small", "fks_simulate_linked_path_jobs_small", "fks_simulate_se2_path_jobs_small",
          "fks_simulate_se3_path_jobs_small"}},
        {POLICY, THROUGHPUT,
         {"fks_simulate_linked_policy", "fks_simulate_linked_lean_policy", "fks_simulate_se2_policy", "fks_simulate_se3_policy"}},
        {POLICY, SMALL,
         {"fks_simulate_linked_policy_small", "fks_simulate_linked_policy_small", "fks_simulate_se2_policy_small",
          "fks_simulate_se3_policy_small"}},
    };
    std::set<int> rows;
    std::set<std::string> names;
    bool listed[FORM_COUNT][BUDGET_COUNT] = {};
    for (const Named& k : kAll) {
        listed[k.form][k.budget] = true;
        for (int family = 0; family < FAMILY_COUNT; ++family) {
            const int row = kernel_row(KernelId{k.form, k.budget, (Family)family});
            EXPECT(row >= 0 && row < kKernelRows);
            const char* name = kernel_symbol(row);
            EXPECT(name && std::strcmp(name, k.names[family]) == 0);
            if (!name || std::strcmp(name, k.names[family]) != 0)
                std::fprintf(stderr, "  form %d budget %d family %d: %s, expected %s\n", k.form, k.budget, family, name ? name : "(none)",
                             k.names[family]);
            rows.insert(row);
            names.insert(k.names[family]);
        }
    }
    EXPECT(rows.size() == 52 && names.size() == 52 && kKernelRows == 52); /* every row of the list is somebody's kernel */
    /* the forms without a small-batch instantiation have none for any family */
    for (int form = 0; form < FORM_COUNT; ++form)
        for (int family = 0; family < FAMILY_COUNT; ++family)
            if (!listed[form][SMALL]) EXPECT(kernel_row(KernelId{(Form)form, SMALL, (Family)family}) == -1);
    EXPECT(kernel_symbol(-1) == nullptr && kernel_symbol(kKernelRows) == nullptr);
    /* an identity that is none of the enumerators has no row */
    EXPECT(kernel_row(KernelId{(Form)FORM_COUNT, THROUGHPUT, LINKED}) == -1 && kernel_row(KernelId{PLAIN, (Budget)3, LINKED}) == -1);
    EXPECT(kernel_row(KernelId{PLAIN, THROUGHPUT, (Family)FAMILY_COUNT}) == -1);
}

int main() {
    test_workgroup_halving();
    test_refusals();
    test_minimum_over_kernels();
    test_pairing();
    test_lean();
    test_hbm_cap();
    test_small_batch();
    test_cooperative();
    test_plain_calls();
    test_checks();
    test_batches();
    test_grid();
    test_register_gates();
    test_kernel_list();
    if (g_failures) {
        std::fprintf(stderr, "%d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("launch plan test ok\n");
    return 0;
}
