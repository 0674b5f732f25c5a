/*
 * batch_plan_test.cpp — the host-side plan of batched calls (csrc/fks_batch.h) without a GPU:
 * the normal form of a path, a job batch and a path-job batch, their refusals, the segment plan
 * and the kernel-argument records.  Small host arrays stand in for the device buffers (the
 * planner offsets and stores the pointers, it never dereferences them).  Links fks_batch.cpp only.
 */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fks_batch.h"

using namespace fks_batch;
using fksd::SimArgs;

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                  \
        }                                                                  \
    } while (0)

constexpr uint32_t W = 3;
constexpr uint64_t kSeed = 0x5eedull, kCall = 100;

static Inputs inputs(uint32_t segment_steps = 0) {
    Inputs in;
    in.seed = kSeed;
    in.call_index = kCall;
    const double frequency = 10.0, time = 2.0;
    in.T = (uint32_t)(time * frequency); /* 20 */
    in.segment_steps = segment_steps;
    in.grid_waves = 4;
    in.small_grid_waves = 2;
    in.W = W;
    in.seg_stride = 7;
    in.heavy_per_step = 2;
    in.heavy_priority = 2;
    in.heavy_relative = 3;
    std::memset(&in.base, 0, sizeof(in.base));
    in.base.dt = 0.1;
    in.base.row_cap = 9;
    return in;
}

/* stand-ins for device buffers */
static double g_starts[64], g_way[256], g_out[256], g_state[1024];
static uint8_t g_coll[64];
static uint32_t g_res[64], g_err[64], g_done[64];

struct Built {
    Batch b;
    RecordPlan rp;
    std::vector<SimArgs> h, d; /* the upload, and where it would lie on the device */
    const uint32_t* first() const { return reinterpret_cast<const uint32_t*>(h.data() + b.legs); }
    const uint32_t* leg_first() const { return first() + b.num_jobs + 1; }
};
static void plan_and_build(const Inputs& in, Built* t) {
    std::string why;
    CHECK(check_arguments(&t->b, in.individual_jacobians, &why) == FKS_OK);
    CHECK(plan_batch(in, &t->b, &why) == FKS_OK);
    t->rp = plan_records(t->b);
    t->h.resize(t->rp.records);
    t->d.resize(t->rp.records);
    std::memset(t->h.data(), 0xab, t->h.size() * sizeof(SimArgs));
    const SegmentPlan& p = t->b.plan;
    if (t->rp.launch)
        build_records(in, t->b, p.seg_state_words ? g_state : nullptr, p.seg_done_words ? g_done : nullptr, t->d.data(), t->h.data());
}
static uint64_t key_of(const SimArgs& r) { return (uint64_t)r.key0 | ((uint64_t)r.key1 << 32); }
static uint64_t call_key(uint64_t call) { return splitmix64(kSeed ^ splitmix64(call)); }

static fks_path_job path_job(uint64_t n, uint64_t legs, uint64_t num_targets, uint64_t at = 0) {
    fks_path_job p;
    std::memset(&p, 0, sizeof(p));
    p.starts = g_starts + at * W;
    p.n = n;
    p.waypoints = g_way + at * W;
    p.num_legs = legs;
    p.num_targets = num_targets;
    p.first_particle_id = 7 * at;
    p.allow_contacts = 1;
    p.out_positions = g_out + at * W;
    p.out_collided = g_coll + at;
    p.out_microsteps = nullptr; /* an optional output the caller does not want */
    p.out_resolver_iterations = g_res + at;
    p.out_error_flags = g_err + at;
    return p;
}
static fks_job job(uint64_t n, uint64_t num_targets, uint64_t at) { return as_job(path_job(n, 1, num_targets, at)); }

/* what a kernel reads of a record whatever its form ... */
static bool same_common(const SimArgs& a, const SimArgs& b) {
    return a.key0 == b.key0 && a.key1 == b.key1 && a.T == b.T && a.starts == b.starts && a.targets == b.targets &&
           a.num_targets == b.num_targets && a.n == b.n && a.first_pid == b.first_pid && a.allow_contacts == b.allow_contacts &&
           a.out_q == b.out_q && a.pid_io == b.pid_io && a.out_collided == b.out_collided && a.out_micro == b.out_micro &&
           a.out_resolver == b.out_resolver && a.out_err == b.out_err && a.seg_state == b.seg_state && a.seg_done == b.seg_done &&
           a.seg_steps == b.seg_steps && a.nseg == b.nseg && a.seg_stride == b.seg_stride &&
           a.seg_heavy_resolver == b.seg_heavy_resolver && a.seg_heavy_prio == b.seg_heavy_prio && a.seg_heavy_rel == b.seg_heavy_rel &&
           a.dt == b.dt && a.row_cap == b.row_cap;
}
/* ... what only the PATH kernels read (under `if constexpr (PATH)`) ... */
static bool same_path_fields(const SimArgs& a, const SimArgs& b) { return a.path_legs == b.path_legs && a.path_carry == b.path_carry; }
/* ... and what only the JOBS kernels read; job_first's contents are compared by the callers */
static bool same_jobs_fields(const SimArgs& a, const SimArgs& b) {
    return a.num_jobs == b.num_jobs && a.job_base == b.job_base && a.jobs_total == b.jobs_total;
}

static void test_path(uint64_t num_targets) {
    const Inputs in = inputs();
    const uint64_t n = 2, legs = 3;
    Built t;
    from_path(&t.b, ENTRY_PATH_DEVICE, g_starts, n, g_way, legs, num_targets, 5, 1, g_out, g_coll, nullptr, g_res, g_err);
    plan_and_build(in, &t);
    CHECK(t.rp.call_advance == 3 && t.rp.particles == 6 && t.rp.launch);
    CHECK(t.rp.records > legs);
    for (uint64_t leg = 0; leg < legs; ++leg) {
        const SimArgs& r = t.h[leg];
        CHECK(key_of(r) == call_key(kCall + leg));
        CHECK(r.targets == g_way + leg * num_targets * W);
        CHECK(r.starts == (leg == 0 ? g_starts : g_out + (leg - 1) * n * W));
        CHECK(r.out_q == g_out + leg * n * W); /* leg-major slices */
        CHECK(r.out_collided == g_coll + leg * n);
        CHECK(r.out_micro == nullptr);
        CHECK(r.out_resolver == g_res + leg * n && r.out_err == g_err + leg * n);
        CHECK(r.path_legs == 3 && r.n == n && r.num_targets == num_targets && r.first_pid == 5 && r.allow_contacts == 1);
        CHECK(r.T == 20 && r.nseg == 1 && r.seg_steps == 20 && r.path_carry == 1);
        CHECK(r.seg_state == nullptr && r.seg_done == g_done); /* three legs: seg_done counts them */
        CHECK(r.dt == 0.1 && r.row_cap == 9);                  /* the shared arguments */
    }
    /* the same path as a one-job path-job batch: every field the PATH kernels read agrees */
    const fks_path_job one = t.b.jobs()[0];
    Built u;
    from_path_jobs(&u.b, &one, 1);
    plan_and_build(in, &u);
    CHECK(u.rp.call_advance == t.rp.call_advance && u.rp.particles == t.rp.particles);
    for (uint64_t leg = 0; leg < legs; ++leg) CHECK(same_common(t.h[leg], u.h[leg]) && same_path_fields(t.h[leg], u.h[leg]));
}

static void test_jobs(uint32_t segment_steps) {
    const Inputs in = inputs(segment_steps);
    const fks_job jobs[3] = {job(2, 2, 0), job(0, 1, 2), job(1, 1, 2)};
    Built t;
    from_jobs(&t.b, jobs, 3);
    plan_and_build(in, &t);
    CHECK(t.rp.call_advance == 3 && t.rp.particles == 3 && t.rp.launch);
    const uint32_t want_first[4] = {0, 2, 2, 3};
    for (int j = 0; j < 4; ++j) CHECK(t.first()[j] == want_first[j]);
    const bool seg = segment_steps != 0;
    CHECK(t.b.plan.nseg == (seg ? 3u : 1u));
    for (uint64_t j = 0; j < 3; ++j) {
        const SimArgs& r = t.h[j];
        CHECK(key_of(r) == call_key(kCall + j));
        CHECK(r.job_base == want_first[j] && r.num_jobs == 3 && r.jobs_total == 3);
        CHECK(r.job_first == reinterpret_cast<const uint32_t*>(t.d.data() + 3));
        /* the slices start at the job's first global particle; null when the plan allocates none */
        CHECK(r.seg_done == (seg ? g_done + want_first[j] : nullptr));
        CHECK(r.seg_state == (seg ? g_state + want_first[j] * in.seg_stride : nullptr));
        CHECK(r.n == jobs[j].n && r.num_targets == jobs[j].num_targets && r.first_pid == jobs[j].first_particle_id);
        if (jobs[j].n == 0) continue; /* an empty job's arrays are never read */
        CHECK(r.starts == jobs[j].starts && r.targets == jobs[j].targets && r.out_q == jobs[j].out_positions);
        CHECK(r.out_collided == jobs[j].out_collided && r.out_micro == nullptr && r.out_err == jobs[j].out_error_flags);
    }
    /* the same jobs as one-leg path jobs: every field the JOBS kernels read agrees */
    fks_path_job pj[3];
    for (int j = 0; j < 3; ++j) pj[j] = t.b.jobs()[j];
    Built u;
    from_path_jobs(&u.b, pj, 3);
    plan_and_build(in, &u);
    CHECK(u.rp.call_advance == 3 && u.rp.particles == 3);
    for (int j = 0; j < 4; ++j) CHECK(u.first()[j] == t.first()[j]);
    for (uint64_t j = 0; j < 3; ++j) CHECK(same_common(t.h[j], u.h[j]) && same_jobs_fields(t.h[j], u.h[j]));
}

static void test_path_jobs() {
    const Inputs in = inputs();
    const fks_path_job jobs[3] = {path_job(1, 2, 1, 0), path_job(0, 1, 1, 4), path_job(2, 3, 2, 8)};
    Built t;
    from_path_jobs(&t.b, jobs, 3);
    plan_and_build(in, &t);
    CHECK(t.rp.call_advance == 6 && t.rp.particles == 1 * 2 + 0 + 2 * 3 && t.rp.launch);
    const uint32_t want_first[4] = {0, 1, 1, 3}, want_leg_first[4] = {0, 2, 3, 6};
    for (int j = 0; j < 4; ++j) CHECK(t.first()[j] == want_first[j] && t.leg_first()[j] == want_leg_first[j]);
    uint64_t rec = 0;
    for (uint64_t j = 0; j < 3; ++j)
        for (uint64_t leg = 0; leg < jobs[j].num_legs; ++leg, ++rec) {
            const SimArgs& r = t.h[rec];
            CHECK(key_of(r) == call_key(kCall + rec)); /* consecutive over (job, leg) */
            CHECK(r.path_legs == jobs[j].num_legs && r.path_legs_max == 3);
            CHECK(r.job_base == want_first[j] && r.num_jobs == 3 && r.jobs_total == 3);
            CHECK(r.job_first == reinterpret_cast<const uint32_t*>(t.d.data() + 6));
            CHECK(r.seg_done == g_done + want_first[j] && r.seg_state == nullptr);
            if (jobs[j].n == 0) continue;
            CHECK(r.starts == (leg == 0 ? jobs[j].starts : jobs[j].out_positions + (leg - 1) * jobs[j].n * W));
            CHECK(r.targets == jobs[j].waypoints + leg * jobs[j].num_targets * W);
            CHECK(r.out_q == jobs[j].out_positions + leg * jobs[j].n * W && r.out_micro == nullptr);
            CHECK(r.out_resolver == jobs[j].out_resolver_iterations + leg * jobs[j].n);
        }
}

static void test_segment_plan() {
    Inputs in = inputs();
    CHECK(plan_segments(in, 3, 1).nseg == 1 && !plan_segments(in, 3, 1).segmented);
    const SegmentPlan p5 = plan_segments(in, 5, 1);
    CHECK(p5.segmented && p5.seg_steps == 14 && p5.nseg == 2 && p5.seg_heavy_resolver == 28 && p5.seg_heavy_prio == 2);
    CHECK(p5.seg_done_words == 5 && p5.seg_state_words == 5 * 7);
    in.segment_steps = 9;
    CHECK(plan_segments(in, 1, 1).nseg == 3 && plan_segments(in, 1000, 1).nseg == 3 && plan_segments(in, 1, 1).seg_steps == 9);
    CHECK(plan_segments(in, 0, 1).nseg == 1 && plan_segments(in, 0, 1).refusal_nseg == 3); /* nothing to segment */
    CHECK(plan_segments(in, 5, 1, /*segmentable=*/false).nseg == 1);                        /* a traced call runs whole */
    in.segment_steps = 50;
    CHECK(plan_segments(in, 1, 1).seg_steps == 20 && plan_segments(in, 1, 1).nseg == 1);
    /* small: small_batch, not individual Jacobians, not lean, one segment, n <= small_grid_waves */
    for (int mask = 0; mask < 32; ++mask) {
        Inputs v = inputs((mask & 8) ? 9 : 0);
        v.small_batch = !(mask & 1);
        v.individual_jacobians = (mask & 2) != 0;
        v.lean = (mask & 4) != 0;
        const uint64_t n = (mask & 16) ? 3 : 2;
        const SegmentPlan p = plan_segments(v, n, 1);
        CHECK(p.small == (v.small_batch && !v.individual_jacobians && !v.lean && p.nseg == 1 && n <= 2));
    }
    /* path_carry: one segment and a wave of the launched grid for every particle */
    in = inputs();
    CHECK(plan_segments(in, 2, 3).path_carry && plan_segments(in, 4, 3).path_carry && !plan_segments(in, 5, 3).path_carry);
    in.segment_steps = 9;
    CHECK(!plan_segments(in, 2, 3).path_carry);
    in.segment_steps = 20; /* explicit, one segment */
    CHECK(plan_segments(in, 2, 3).path_carry && plan_segments(in, 2, 3).seg_done_words == 2);
    /* the relative heavy test switches off at n x nseg x legs >= 2^24 */
    in.segment_steps = 10; /* nseg = 2 */
    CHECK(plan_segments(in, (1ull << 21) - 1, 4).seg_heavy_rel == 3);
    CHECK(plan_segments(in, 1ull << 21, 4).seg_heavy_rel == 0);
}

static void refused(Batch* b, const Inputs& in, fks_status st, const char* text) {
    std::string why;
    fks_status got = check_arguments(b, in.individual_jacobians, &why);
    if (got == FKS_OK) got = plan_batch(in, b, &why);
    if (got != st || why != text) {
        std::fprintf(stderr, "refusal: want %d \"%s\", got %d \"%s\"\n", (int)st, text, (int)got, why.c_str());
        ++g_failures;
    }
}

static void test_refusals() {
    const Inputs in = inputs();
    Inputs indiv = inputs();
    indiv.individual_jacobians = true;
    Inputs fine = inputs(1); /* one step per segment over many steps: 40000 segments per leg */
    fine.T = 40000;
    const uint64_t big = 0xffffffffull;
    const fks_status INV = FKS_ERR_INVALID_ARGUMENT;
    Batch b;
    /* a path through the device entry ... */
    from_path(&b, ENTRY_PATH_DEVICE, g_starts, 2, g_way, 0, 1, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, indiv, INV, "a path needs at least one leg"); /* wins over the individual Jacobians */
    from_path(&b, ENTRY_PATH_DEVICE, g_starts, 2, g_way, 3, 1, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, indiv, FKS_ERR_UNSUPPORTED, "no path kernel with individual Jacobians (fks_set_individual_jacobians): chain plain calls");
    from_path(&b, ENTRY_PATH_DEVICE, g_starts, 2, nullptr, 3, 5, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, in, INV, "null device buffer"); /* wins over the targets */
    from_path(&b, ENTRY_PATH_DEVICE, g_starts, 2, g_way, 3, 5, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, in, INV, "targets must be 1 or n (SPCS:792)");
    from_path(&b, ENTRY_PATH_DEVICE, g_starts, big + 1, g_way, 3, 1, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, in, INV, "at most 2^32-1 particles per call");
    from_path(&b, ENTRY_PATH_DEVICE, g_starts, 2, g_way, 1ull << 30, 1, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, inputs(9), INV, "legs x segments per leg must stay below 2^31");
    from_path(&b, ENTRY_PATH_DEVICE, nullptr, 0, nullptr, 1ull << 30, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
    refused(&b, inputs(9), INV, "legs x segments per leg must stay below 2^31"); /* an empty path as a full one */
    /* ... and through the host entry */
    from_path(&b, ENTRY_PATH_HOST, nullptr, 2, g_way, 3, 1, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, in, INV, "null host buffer");
    from_path(&b, ENTRY_PATH_HOST, g_starts, 2, g_way, 3, 5, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, in, INV, "waypoints must hold 1 or n configurations per leg (SPCS:792)");
    from_path(&b, ENTRY_PATH_HOST, g_starts, big + 1, g_way, 3, 1, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, in, INV, "path too large");
    from_path(&b, ENTRY_PATH_HOST, g_starts, 2, g_way, 1ull << 31, 1, 0, 1, g_out, nullptr, nullptr, nullptr, nullptr);
    refused(&b, in, INV, "path too large");
    /* a job batch */
    fks_job jobs[2] = {job(2, 1, 0), job(2, 2, 2)};
    from_jobs(&b, jobs, 0);
    refused(&b, in, INV, "a job batch needs at least one job");
    from_jobs(&b, nullptr, 2);
    refused(&b, in, INV, "a job batch needs at least one job");
    from_jobs(&b, jobs, 65537); /* refused by its count: the array is not read */
    refused(&b, indiv, INV, "at most 65536 jobs per batch");
    from_jobs(&b, jobs, 2);
    refused(&b, indiv, FKS_ERR_UNSUPPORTED, "no jobs kernel with individual Jacobians (fks_set_individual_jacobians): issue plain calls");
    jobs[1].num_targets = 5;
    jobs[1].starts = nullptr;
    from_jobs(&b, jobs, 2);
    refused(&b, in, INV, "job 1: targets must be 1 or n (SPCS:792)"); /* wins over the null buffer */
    jobs[1].num_targets = 2;
    from_jobs(&b, jobs, 2);
    refused(&b, in, INV, "job 1: null starts, targets or out_positions");
    jobs[1] = job(big - 1, 1, 2);
    from_jobs(&b, jobs, 2);
    refused(&b, in, INV, "at most 2^32-1 particles per batch");
    jobs[1] = job(2, 2, 2);
    from_jobs(&b, jobs, 2);
    {
        std::string why;
        CHECK(check_arguments(&b, false, &why) == FKS_OK && plan_batch(fine, &b, &why) == FKS_OK); /* one leg each: no 2^31 bound */
        CHECK(b.plan.nseg == 40000);
    }
    /* a path-job batch */
    fks_path_job pj[2] = {path_job(2, 2, 1, 0), path_job(2, 3, 2, 4)};
    from_path_jobs(&b, pj, 0);
    refused(&b, in, INV, "a path-job batch needs at least one job");
    from_path_jobs(&b, nullptr, 2);
    refused(&b, in, INV, "a path-job batch needs at least one job");
    from_path_jobs(&b, pj, 65537);
    refused(&b, indiv, INV, "at most 65536 jobs per batch");
    from_path_jobs(&b, pj, 2);
    refused(&b, indiv, FKS_ERR_UNSUPPORTED, "no path-jobs kernel with individual Jacobians (fks_set_individual_jacobians): issue plain calls");
    pj[0].num_legs = 0;
    refused(&b, in, INV, "job 0: a path needs at least one leg");
    pj[0].num_legs = 65536;
    refused(&b, in, INV, "at most 65536 legs per batch (the sum of num_legs)"); /* 65536 + 3 */
    pj[0].num_legs = 65537;
    refused(&b, in, INV, "at most 65536 legs per batch (the sum of num_legs)");
    pj[0].num_legs = 2;
    pj[1].num_targets = 5;
    pj[1].waypoints = nullptr;
    refused(&b, in, INV, "job 1: waypoints must hold 1 or n configurations per leg (SPCS:792)");
    pj[1].num_targets = 2;
    refused(&b, in, INV, "job 1: null starts, waypoints or out_positions");
    pj[1] = path_job(big - 1, 3, 1, 4);
    refused(&b, in, INV, "at most 2^32-1 particles per batch");
    pj[1] = path_job(2, 65000, 2, 4);
    refused(&b, fine, INV, "legs x segments per leg must stay below 2^31"); /* 65000 x 40000 */
}

static void test_empty_batches() {
    const Inputs in = inputs();
    Built p;
    from_path(&p.b, ENTRY_PATH_DEVICE, nullptr, 0, nullptr, 4, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
    plan_and_build(in, &p);
    CHECK(!p.rp.launch && p.rp.call_advance == 4 && p.rp.particles == 0);
    const fks_job jobs[2] = {job(0, 1, 0), job(0, 0, 0)};
    Built j;
    from_jobs(&j.b, jobs, 2);
    plan_and_build(in, &j);
    CHECK(!j.rp.launch && j.rp.call_advance == 2 && j.rp.particles == 0);
    const fks_path_job pj[2] = {path_job(0, 2, 1), path_job(0, 3, 1)};
    Built q;
    from_path_jobs(&q.b, pj, 2);
    plan_and_build(in, &q);
    CHECK(!q.rp.launch && q.rp.call_advance == 5 && q.rp.particles == 0);
}

int main() {
    test_path(1);
    test_path(2);
    test_jobs(0);
    test_jobs(9);
    test_path_jobs();
    test_segment_plan();
    test_refusals();
    test_empty_batches();
    if (g_failures) {
        std::fprintf(stderr, "batch plan test: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("batch plan test ok\n");
    return 0;
}
