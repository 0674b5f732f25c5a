/*
 * fks_batch.cpp — the normal form, checks, segment plan and records of batched calls (fks_batch.h).
 * Host only: no HIP runtime call.
 */
#include "fks_batch.h"

#include <algorithm>
#include <cstring>

namespace fks_batch {

uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

SegmentPlan plan_segments(const Inputs& in, uint64_t n, uint64_t legs, bool segmentable) {
    /* controller-step segments: automatically only when the batch outnumbers the
     * resident waves (otherwise every particle has a wave from the start), always
     * when set explicitly (fks_set_segment_steps); traced calls run whole */
    SegmentPlan p;
    const uint32_t k = std::min(in.segment_steps ? in.segment_steps : kDefaultSegmentSteps, in.T);
    /* T >= 1 and k >= 1: ceil(T / k) without the uint32 wrap of (T + k - 1) / k */
    const uint64_t per_leg = ((uint64_t)in.T - 1u) / k + 1u;
    const bool wanted = in.segment_steps != 0 || n > (uint64_t)in.grid_waves;
    p.refusal_nseg = wanted ? per_leg : 1u;
    p.segmented = segmentable && n > 0 && wanted;
    p.seg_steps = p.segmented ? k : in.T;
    p.nseg = p.segmented ? (uint32_t)per_leg : 1u;
    if (p.segmented) {
        /* heavy_per_step <= 65536 (fks_set_segment_policy): the product fits in 64 bits,
         * and the kernel compares it with a per-segment count of at most 2^32 - 1 */
        const uint64_t heavy = (uint64_t)in.heavy_per_step * k;
        p.seg_heavy_resolver = (uint32_t)std::min<uint64_t>(heavy, 0xffffffffull);
        p.seg_heavy_prio = in.heavy_priority;
        /* the relative test's running sums pack 24 bits of segments: off for larger batches */
        p.seg_heavy_rel = ((uint64_t)n * p.nseg * legs < (1ull << 24)) ? in.heavy_relative : 0u;
    }
    /* a batch that fits the small-batch kernel's resident waves, whole particles, plain
     * simulation: that kernel (every particle has its wave from the start either way) */
    p.small = in.small_batch && !in.individual_jacobians && !in.lean && p.nseg == 1 && n <= (uint64_t)in.small_grid_waves;
    p.path_carry = p.nseg == 1 && n <= (uint64_t)(p.small ? in.small_grid_waves : in.grid_waves);
    /* seg_done counts a particle's legs x nseg segments, so it is needed from two legs on;
     * the resting state only between the segments of a leg */
    if ((uint64_t)p.nseg * legs > 1) p.seg_done_words = n;
    if (p.nseg > 1) p.seg_state_words = n * (uint64_t)in.seg_stride;
    return p;
}

void apply_segments(const SegmentPlan& p, fksd::SimArgs* a) {
    a->seg_steps = p.seg_steps;
    a->nseg = p.nseg;
    a->seg_heavy_resolver = p.seg_heavy_resolver;
    a->seg_heavy_prio = p.seg_heavy_prio;
    a->seg_heavy_rel = p.seg_heavy_rel;
}

void from_path(Batch* b, Entry entry, const double* starts, uint64_t n, const double* waypoints, uint64_t num_legs,
               uint64_t num_targets, uint64_t first_particle_id, int32_t allow_contacts, double* out_positions,
               uint8_t* out_collided, uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags) {
    b->form = PATH;
    b->entry = entry;
    b->num_jobs = 1;
    b->converted.resize(1);
    fks_path_job& p = b->converted[0];
    std::memset(&p, 0, sizeof(p));
    p.starts = starts;
    p.n = n;
    p.waypoints = waypoints;
    p.num_legs = num_legs;
    p.num_targets = num_targets;
    p.first_particle_id = first_particle_id;
    p.allow_contacts = allow_contacts;
    p.out_positions = out_positions;
    p.out_collided = out_collided;
    p.out_microsteps = out_microsteps;
    p.out_resolver_iterations = out_resolver_iterations;
    p.out_error_flags = out_error_flags;
}

void from_policy(Batch* b, Entry entry, const double* starts, uint64_t n, const fks_policy_table* table, uint64_t max_legs,
                 uint64_t first_particle_id, int32_t allow_contacts, double* out_positions, uint8_t* out_collided,
                 uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags, uint32_t* out_choice,
                 double* out_distance, uint32_t* out_legs_run) {
    /* a path whose legs' targets are chosen on the device: no waypoints, a target per particle */
    from_path(b, entry, starts, n, nullptr, max_legs, n, first_particle_id, allow_contacts, out_positions, out_collided,
              out_microsteps, out_resolver_iterations, out_error_flags);
    b->policy = true;
    b->has_table = table != nullptr;
    if (table) b->table = *table;
    b->out_choice = out_choice;
    b->out_distance = out_distance;
    b->out_legs_run = out_legs_run;
}

void from_jobs(Batch* b, const fks_job* jobs, uint64_t num_jobs) {
    b->form = JOBS;
    b->entry = ENTRY_JOBS;
    b->num_jobs = jobs ? num_jobs : 0;
    b->converted.clear();
    if (b->num_jobs > FKS_MAX_JOBS) return; /* refused by its count: the array is not read */
    b->converted.resize((size_t)b->num_jobs);
    for (size_t j = 0; j < b->converted.size(); ++j) {
        const fks_job& job = jobs[j];
        fks_path_job& p = b->converted[j];
        std::memset(&p, 0, sizeof(p));
        p.starts = job.starts;
        p.n = job.n;
        p.waypoints = job.targets;
        p.num_legs = 1;
        p.num_targets = job.num_targets;
        p.first_particle_id = job.first_particle_id;
        p.allow_contacts = job.allow_contacts;
        p.out_positions = job.out_positions;
        p.out_collided = job.out_collided;
        p.out_microsteps = job.out_microsteps;
        p.out_resolver_iterations = job.out_resolver_iterations;
        p.out_error_flags = job.out_error_flags;
    }
}

void from_path_jobs(Batch* b, const fks_path_job* jobs, uint64_t num_jobs) {
    b->form = PATH_JOBS;
    b->entry = ENTRY_PATH_JOBS;
    b->num_jobs = jobs ? num_jobs : 0;
    b->converted.clear();
    b->external = jobs;
}

fks_job as_job(const fks_path_job& p) {
    fks_job job;
    std::memset(&job, 0, sizeof(job));
    job.starts = p.starts;
    job.n = p.n;
    job.targets = p.waypoints;
    job.num_targets = p.num_targets;
    job.first_particle_id = p.first_particle_id;
    job.allow_contacts = p.allow_contacts;
    job.out_positions = p.out_positions;
    job.out_collided = p.out_collided;
    job.out_microsteps = p.out_microsteps;
    job.out_resolver_iterations = p.out_resolver_iterations;
    job.out_error_flags = p.out_error_flags;
    return job;
}

namespace {

/* the refusals that read differently per entry; a null text: the entry has no such refusal */
struct Wording {
    const char* no_jobs;
    const char* individual;
    const char* targets;
    const char* null_buffer;
    const char* particles;
    const char* too_large; /* n or the legs past what the host path entry stages */
};
const char* const kWaypointsOneOrN = "waypoints must hold 1 or n configurations per leg (SPCS:792)";
const char* const kNoPathKernel = "no path kernel with individual Jacobians (fks_set_individual_jacobians): chain plain calls";
const char* const kNoPolicyKernel = "no policy kernel with individual Jacobians (fks_set_individual_jacobians): chain plain calls";
const Wording kWording[] = {
    /* ENTRY_PATH_DEVICE */
    {nullptr, kNoPathKernel, kTargetsOneOrN, "null device buffer", "at most 2^32-1 particles per call", nullptr},
    /* ENTRY_PATH_HOST */
    {nullptr, kNoPathKernel, kWaypointsOneOrN, "null host buffer", "at most 2^32-1 particles per call",
     "path too large"},
    /* ENTRY_JOBS */
    {"a job batch needs at least one job", "no jobs kernel with individual Jacobians (fks_set_individual_jacobians): issue plain calls",
     kTargetsOneOrN, "null starts, targets or out_positions", "at most 2^32-1 particles per batch", nullptr},
    /* ENTRY_PATH_JOBS */
    {"a path-job batch needs at least one job",
     "no path-jobs kernel with individual Jacobians (fks_set_individual_jacobians): issue plain calls",
     kWaypointsOneOrN, "null starts, waypoints or out_positions",
     "at most 2^32-1 particles per batch", nullptr},
    /* ENTRY_POLICY_DEVICE */
    {nullptr, kNoPolicyKernel, nullptr, "null device buffer (starts, out_positions or out_choice)",
     "at most 2^32-1 particles per call", nullptr},
    /* ENTRY_POLICY_HOST */
    {nullptr, kNoPolicyKernel, nullptr, "null host buffer (starts, out_positions or out_choice)",
     "at most 2^32-1 particles per call", "roll-out too large"},
};

fks_status refuse(std::string* why, fks_status st, std::string text) {
    *why = std::move(text);
    return st;
}

/* a roll-out's refusals: its legs, its table, its buffers, then its size */
fks_status check_policy(Batch* b, bool individual_jacobians, std::string* why) {
    const Wording& w = kWording[b->entry];
    const fks_path_job& job = b->jobs()[0];
    const fks_policy_table& t = b->table;
    if (job.num_legs == 0) return refuse(why, FKS_ERR_INVALID_ARGUMENT, "a roll-out needs at least one leg (max_legs)");
    if (individual_jacobians) return refuse(why, FKS_ERR_UNSUPPORTED, w.individual);
    if (!b->has_table) return refuse(why, FKS_ERR_INVALID_ARGUMENT, "null policy table");
    if (t.num_entries == 0) return refuse(why, FKS_ERR_INVALID_ARGUMENT, "a policy table needs at least one entry");
    if (t.num_entries > FKS_MAX_POLICY_ENTRIES) return refuse(why, FKS_ERR_INVALID_ARGUMENT, "at most 2^30 policy entries");
    if (!t.keys || !t.targets) return refuse(why, FKS_ERR_INVALID_ARGUMENT, "null policy keys or targets");
    if (t.terminal_distance != t.terminal_distance || t.max_distance != t.max_distance)
        return refuse(why, FKS_ERR_INVALID_ARGUMENT, "terminal_distance or max_distance is NaN");
    if (job.n > 0 && (!job.starts || !job.out_positions || !b->out_choice)) return refuse(why, FKS_ERR_INVALID_ARGUMENT, w.null_buffer);
    if (w.too_large && (job.n > 0xffffffffull || job.num_legs >= (1ull << 31))) return refuse(why, FKS_ERR_INVALID_ARGUMENT, w.too_large);
    if (job.n > 0xffffffffull) return refuse(why, FKS_ERR_INVALID_ARGUMENT, w.particles);
    b->total = job.n;
    b->legs = b->max_legs = job.num_legs;
    b->rows = job.n * job.num_legs;
    return FKS_OK;
}

}  // namespace

fks_status check_arguments(Batch* b, bool individual_jacobians, std::string* why) {
    if (b->policy) return check_policy(b, individual_jacobians, why);
    const Wording& w = kWording[b->entry];
    const bool one_path = b->form == PATH; /* a path's checks name no job, and hold from one particle on */
    if (one_path) {
        if (b->jobs()[0].num_legs == 0) return refuse(why, FKS_ERR_INVALID_ARGUMENT, "a path needs at least one leg");
    } else {
        if (b->num_jobs == 0) return refuse(why, FKS_ERR_INVALID_ARGUMENT, w.no_jobs);
        if (b->num_jobs > FKS_MAX_JOBS) return refuse(why, FKS_ERR_INVALID_ARGUMENT, "at most 65536 jobs per batch");
    }
    if (individual_jacobians) return refuse(why, FKS_ERR_UNSUPPORTED, w.individual);
    b->total = b->legs = b->max_legs = b->rows = 0;
    for (uint64_t j = 0; j < b->num_jobs; ++j) {
        const fks_path_job& job = b->jobs()[j];
        const bool bad_targets = job.num_targets != 1 && job.num_targets != job.n;
        const bool null_buffer = job.n > 0 && (!job.starts || !job.waypoints || !job.out_positions);
        if (one_path) {
            if (null_buffer) return refuse(why, FKS_ERR_INVALID_ARGUMENT, w.null_buffer);
            if (job.n > 0 && bad_targets) return refuse(why, FKS_ERR_INVALID_ARGUMENT, w.targets);
            if (w.too_large && (job.n > 0xffffffffull || job.num_legs >= (1ull << 31)))
                return refuse(why, FKS_ERR_INVALID_ARGUMENT, w.too_large);
        } else {
            const auto who = [j]() { return "job " + std::to_string(j) + ": "; };
            if (job.num_legs == 0) return refuse(why, FKS_ERR_INVALID_ARGUMENT, who() + "a path needs at least one leg");
            if (job.num_legs > FKS_MAX_PATH_JOB_LEGS || b->legs + job.num_legs > FKS_MAX_PATH_JOB_LEGS)
                return refuse(why, FKS_ERR_INVALID_ARGUMENT, "at most 65536 legs per batch (the sum of num_legs)");
            if (bad_targets) return refuse(why, FKS_ERR_INVALID_ARGUMENT, who() + w.targets);
            if (null_buffer) return refuse(why, FKS_ERR_INVALID_ARGUMENT, who() + w.null_buffer);
        }
        if (job.n > 0xffffffffull || b->total + job.n > 0xffffffffull) return refuse(why, FKS_ERR_INVALID_ARGUMENT, w.particles);
        b->total += job.n;
        b->legs += job.num_legs;
        b->max_legs = std::max<uint64_t>(b->max_legs, job.num_legs);
        b->rows += job.n * job.num_legs; /* path jobs: < 2^32 x 2^16 */
    }
    return FKS_OK;
}

fks_status plan_batch(const Inputs& in, Batch* b, std::string* why) {
    b->plan = plan_segments(in, b->total, b->max_legs);
    /* seg_done counts a particle's segments over all legs (the longest job's) in 31 bits (the top
     * bit marks a claim); a job batch's legs are one each */
    if (b->form != JOBS && (b->max_legs >= (1ull << 31) || b->max_legs * b->plan.refusal_nseg >= (1ull << 31)))
        return refuse(why, FKS_ERR_INVALID_ARGUMENT, "legs x segments per leg must stay below 2^31");
    return FKS_OK;
}

RecordPlan plan_records(const Batch& b) {
    RecordPlan r;
    /* the records are followed by job_first and leg_first [num_jobs + 1], in whole records */
    const size_t prefix = (2 * (size_t)(b.num_jobs + 1) * sizeof(uint32_t) + sizeof(fksd::SimArgs) - 1) / sizeof(fksd::SimArgs);
    r.records = (size_t)b.legs + prefix;
    static_assert(sizeof(fksd::PolicyArgs) <= sizeof(fksd::SimArgs), "a roll-out's PolicyArgs takes one unit of the upload");
    if (b.policy) r.policy_record = r.records++;
    r.call_advance = b.legs; /* a path's legs, a job batch's jobs, a path-job batch's sum of legs */
    /* the counters are the chain's sums; a roll-out's chain simulates the pairs its kernel counts */
    r.particles = b.policy ? 0 : b.rows;
    r.launch = b.total > 0;  /* the chain's calls would launch nothing either */
    return r;
}

void build_records(const Inputs& in, const Batch& b, double* seg_state, uint32_t* seg_done, const fksd::SimArgs* d_records,
                   fksd::SimArgs* h_records) {
    /* job-major, one record per (job, leg): the same call over all particles except for what a
     * leg owns (the key of the sequence's call index, its waypoints, its start configurations:
     * the leg before's output slice, and its slices of the leg-major outputs) and what a job
     * owns (its arguments, and its slices of the segment arrays, which start at the job's first
     * global particle); the two prefix arrays follow the records in the same upload */
    const uint64_t W = (uint64_t)in.W;
    fksd::SimArgs a = in.base;
    a.T = in.T;
    a.seg_stride = in.seg_stride;
    apply_segments(b.plan, &a);
    a.seg_state = seg_state;
    a.seg_done = seg_done;
    a.path_carry = b.plan.path_carry ? 1u : 0u;
    a.path_legs_max = (uint32_t)b.max_legs;
    a.job_first = reinterpret_cast<const uint32_t*>(d_records + b.legs);
    a.num_jobs = (uint32_t)b.num_jobs;
    a.jobs_total = b.total;
    uint32_t* h_first = reinterpret_cast<uint32_t*>(h_records + b.legs);
    uint32_t* h_leg_first = h_first + b.num_jobs + 1;
    uint64_t base = 0, rec = 0;
    for (uint64_t j = 0; j < b.num_jobs; ++j) {
        const fks_path_job& job = b.jobs()[j];
        h_first[j] = (uint32_t)base;
        h_leg_first[j] = (uint32_t)rec;
        for (uint64_t leg = 0; leg < job.num_legs; ++leg) {
            fksd::SimArgs& r = h_records[rec + leg];
            r = a;
            const uint64_t key = splitmix64(in.seed ^ splitmix64(in.call_index + rec + leg));
            r.key0 = (uint32_t)key;
            r.key1 = (uint32_t)(key >> 32);
            r.path_legs = (uint32_t)job.num_legs;
            r.num_targets = job.num_targets;
            r.n = job.n;
            r.first_pid = job.first_particle_id;
            r.allow_contacts = job.allow_contacts ? 1 : 0;
            r.seg_state = seg_state ? seg_state + base * a.seg_stride : nullptr;
            r.seg_done = seg_done ? seg_done + base : nullptr;
            r.job_base = (uint32_t)base;
            if (job.n == 0) continue; /* never read: no particle maps to an empty job */
            r.targets = b.policy ? nullptr : job.waypoints + leg * job.num_targets * W;
            r.starts = leg == 0 ? job.starts : job.out_positions + (leg - 1) * job.n * W;
            r.out_q = job.out_positions + leg * job.n * W;
            r.out_collided = job.out_collided ? job.out_collided + leg * job.n : nullptr;
            r.out_micro = job.out_microsteps ? job.out_microsteps + leg * job.n : nullptr;
            r.out_resolver = job.out_resolver_iterations ? job.out_resolver_iterations + leg * job.n : nullptr;
            r.out_err = job.out_error_flags ? job.out_error_flags + leg * job.n : nullptr;
        }
        base += job.n;
        rec += job.num_legs;
    }
    h_first[b.num_jobs] = (uint32_t)base; /* == total */
    h_leg_first[b.num_jobs] = (uint32_t)rec;
    if (b.policy) {
        fksd::PolicyArgs p;
        std::memset(&p, 0, sizeof(p));
        p.keys = b.table.keys;
        p.targets = b.table.targets;
        p.flags = b.table.flags;
        p.num_entries = b.table.num_entries;
        p.terminal_distance = b.table.terminal_distance;
        p.max_distance = b.table.max_distance;
        p.out_choice = b.out_choice;
        p.out_distance = b.out_distance;
        p.out_legs_run = b.out_legs_run;
        std::memcpy(h_records + plan_records(b).policy_record, &p, sizeof(p));
    }
}

}  // namespace fks_batch

namespace fks_batch {

fks_status plan_cluster(ClusterPlan* p, const double* configs, const uint64_t* group_begin, uint64_t num_groups, double threshold,
                        const void* out_distances, const void* out_labels, const void* out_num_clusters, std::string* why) {
    *p = ClusterPlan();
    auto refuse = [&](const char* text) {
        *why = text;
        return FKS_ERR_INVALID_ARGUMENT;
    };
    if (!(threshold == threshold)) return refuse("threshold is NaN");
    if (!out_distances && !out_labels && !out_num_clusters) return refuse("no output: out_distances, out_labels and out_num_clusters are all NULL");
    if (num_groups >= kMaxClusterConfigs) return refuse("at most 2^31-1 groups per call");
    if (num_groups > 0 && !group_begin) return refuse("null group_begin");
    p->num_groups = num_groups;
    p->labelled = out_labels || out_num_clusters;
    p->launch = num_groups > 0;
    if (num_groups == 0) return FKS_OK;
    /* every offset is checked before any is used: nothing is staged before a refusal */
    for (uint64_t g = 0; g < num_groups; ++g)
        if (group_begin[g + 1] < group_begin[g]) return refuse("group_begin must be ascending");
    p->total = group_begin[num_groups];
    if (p->total > kMaxClusterConfigs) return refuse("at most 2^31 configurations per call");
    p->mat_begin.resize((size_t)num_groups + 1);
    uint64_t words = 0;
    for (uint64_t g = 0; g < num_groups; ++g) {
        const uint64_t n = group_begin[g + 1] - group_begin[g]; /* <= 2^31: n x n fits 64 bits */
        p->mat_begin[(size_t)g] = words;
        p->largest = std::max(p->largest, n);
        if (p->labelled && n > FKS_MAX_CLUSTER_GROUP) return refuse("a group with labels or counts holds at most FKS_MAX_CLUSTER_GROUP (256) configurations");
        if (n > kMaxClusterMatrixWords || words + n * n > kMaxClusterMatrixWords) return refuse("the groups' matrices hold at most 2^27 doubles together");
        words += n * n;
    }
    p->mat_begin[(size_t)num_groups] = words;
    if (group_begin[num_groups] > group_begin[0] && !configs) return refuse("null configs");
    if (p->labelled && p->largest > kClusterLdsGroup) p->work_words = words;
    return FKS_OK;
}

fks_status plan_summary(SummaryPlan* p, int32_t robot_type, uint32_t width, const double* configs, const uint64_t* group_begin,
                        uint64_t num_groups, const uint32_t* labels, const double* targets, double reached_distance,
                        const fks_cluster_summary* out, std::string* why) {
    *p = SummaryPlan();
    auto refuse = [&](const char* text) {
        *why = text;
        return FKS_ERR_INVALID_ARGUMENT;
    };
    if (!out) return refuse("null summary");
    if (!out->order && !out->members && !out->count && !out->begin && !out->expectation && !out->variances && !out->variance &&
        !out->reached)
        return refuse("no output: every pointer of the summary is NULL");
    if (out->reached && !targets) return refuse("reached is asked for without targets");
    if (targets && !out->reached) return refuse("targets are given without reached");
    if (targets && !(reached_distance == reached_distance)) return refuse("reached_distance is NaN");
    if (num_groups >= kMaxClusterConfigs) return refuse("at most 2^31-1 groups per call");
    if (num_groups > 0 && !group_begin) return refuse("null group_begin");
    p->num_groups = num_groups;
    p->launch = num_groups > 0;
    p->width = width;
    p->var_width = fksd::summary_var_width(robot_type, width);
    p->piece_width = fksd::summary_piece_width(robot_type, width);
    /* every index the kernels use in a member's row lies inside the row (a row past it is another group's) */
    if (fksd::summary_row_end(robot_type, width) > p->piece_width) return refuse("internal: a member's terms exceed its workspace row");
    if (num_groups == 0) return FKS_OK;
    /* every offset is checked before any is used: nothing is staged before a refusal */
    for (uint64_t g = 0; g < num_groups; ++g)
        if (group_begin[g + 1] < group_begin[g]) return refuse("group_begin must be ascending");
    p->total = group_begin[num_groups];
    p->first = group_begin[0];
    if (p->total > kMaxClusterConfigs) return refuse("at most 2^31 configurations per call");
    for (uint64_t g = 0; g < num_groups; ++g)
        if (group_begin[g + 1] - group_begin[g] > FKS_MAX_CLUSTER_GROUP)
            return refuse("a group holds at most FKS_MAX_CLUSTER_GROUP (256) configurations");
    if (p->total > 0 && !configs) return refuse("null configs");
    if (p->total > 0 && !labels) return refuse("null labels");
    p->work_words = p->total * ((uint64_t)p->piece_width + width);
    return FKS_OK;
}

fks_status plan_select(SelectPlan* p, uint32_t width, int32_t compute_units, const fks_state_table* table, const double* queries,
                       uint64_t num_queries, uint32_t num_particles, const fks_state_selection* out, std::string* why) {
    *p = SelectPlan();
    auto refuse = [&](const char* text) {
        *why = text;
        return FKS_ERR_INVALID_ARGUMENT;
    };
    if (!table) return refuse("null state table");
    if (!out) return refuse("null selection");
    if (!table->keys) return refuse("null keys");
    if (table->num_states == 0) return refuse("a state table holds at least one state");
    if (table->num_states > FKS_MAX_STATES) return refuse("at most FKS_MAX_STATES (2^30) states");
    if (num_queries > 0 && !out->choice) return refuse("null choice");
    if (num_queries > 0 && !queries) return refuse("null queries");
    const bool draw = out->starts || out->source;
    if (draw && num_particles == 0) return refuse("starts or source is asked for with num_particles == 0");
    if (draw && (!table->count || !table->begin || !table->members))
        return refuse("starts or source is asked for without count, begin and members");
    if (table->begin && !table->count) return refuse("begin is given without count");
    if (num_queries > kMaxSelectQueries) return refuse("at most 2^20 queries per call");
    if (num_particles > kMaxSelectParticles) return refuse("at most 65536 particles per job");
    if (num_queries * (uint64_t)num_particles > kMaxSelectStarts) return refuse("at most 2^31 starts (queries x particles) per call");
    p->num_queries = num_queries;
    p->num_states = table->num_states;
    p->width = width;
    p->particles = num_particles;
    p->draw = draw;
    p->launch = num_queries > 0;
    if (!p->launch) return FKS_OK;
    const uint64_t S = table->num_states, T = fksd::kSelectTile, B = fksd::kSelectThreads;
    p->tile = (uint32_t)std::min<uint64_t>(T, num_queries);
    p->tiles = (num_queries + T - 1) / T;
    const uint64_t cus = (uint64_t)std::max<int32_t>(compute_units, 1);
    const uint64_t wanted = (kSelectGroupsPerCu * cus + p->tiles - 1) / p->tiles;
    const uint64_t blocks = (S + B - 1) / B;
    const uint64_t cut = std::min(wanted, blocks);
    const uint64_t per = (S + cut - 1) / cut;
    p->chunk_states = B * ((per + B - 1) / B);
    p->chunks = (S + p->chunk_states - 1) / p->chunk_states;
    p->groups = p->tiles * p->chunks;
    p->work_partials = num_queries * p->chunks;
    return FKS_OK;
}

}  // namespace fks_batch
