/*
 * fks_batch.h — the host-side plan of a batched call (fks_forward_simulate_path, _jobs,
 * _path_jobs and _policy, on one context or sharded): one normal form for the four entries,
 * their argument checks, the controller-step segment plan and the kernel-argument records.
 *
 * Nothing here calls the HIP runtime or reads an fks_context: the inputs come in a small struct,
 * device pointers are only offset and stored, never dereferenced, so the unit is built and
 * tested on a machine without a GPU (tests/cpp/batch_plan_test.cpp).
 */
#ifndef FKS_BATCH_H
#define FKS_BATCH_H

#include <hip/hip_vector_types.h> /* the vector types SimArgs names */
#include <stdint.h>

#include <string>
#include <vector>

#include "fks_capi.h"
#include "fks_device.h"

namespace fks_batch {

/* controller steps per segment when a batch outnumbers the resident waves: short
 * enough that a contact-heavy particle progresses from the start of the launch, long
 * enough that the hand-over (resting state + one FK) costs < 1 % */
constexpr uint32_t kDefaultSegmentSteps = 14; /* re-swept in round 6: profiles/r06p_sched_ab_cfg*.json */

uint64_t splitmix64(uint64_t x);

/* the refusal of a num_targets that is neither 1 nor n, as the plain calls word it too */
constexpr const char* kTargetsOneOrN = "targets must be 1 or n (SPCS:792)";

/* the kernels a batch runs: PATH reads one record per leg, JOBS one per job, PATH_JOBS one per
 * (job, leg) through both prefix arrays (fks_device.h, SimArgs) */
enum Form { PATH = 0, JOBS = 1, PATH_JOBS = 2 };

/* the entry a batch came through: the row of its refusals' wording (fks_batch.cpp) */
enum Entry { ENTRY_PATH_DEVICE = 0, ENTRY_PATH_HOST, ENTRY_JOBS, ENTRY_PATH_JOBS, ENTRY_POLICY_DEVICE, ENTRY_POLICY_HOST };

/* what the plan reads of a context */
struct Inputs {
    uint64_t seed = 0, call_index = 0;
    uint32_t T = 1;             /* controller steps of a call (forward_steps) */
    uint32_t segment_steps = 0; /* fks_set_segment_steps (0: automatic) */
    uint32_t grid_waves = 0, small_grid_waves = 0;
    bool small_batch = true, individual_jacobians = false, lean = false;
    uint32_t W = 0;          /* R.W: doubles per configuration */
    uint32_t seg_stride = 0; /* doubles per particle in seg_state */
    uint32_t heavy_per_step = 0, heavy_priority = 0, heavy_relative = 0; /* fks_set_segment_policy / _heavy_relative */
    fksd::SimArgs base;      /* everything a record shares with a plain call's arguments */
};

/* controller-step segments of one launch over n particles of `legs` legs each */
struct SegmentPlan {
    bool segmented = false;
    uint32_t seg_steps = 1, nseg = 1;
    uint64_t refusal_nseg = 1; /* segments per leg as the 2^31 refusal counts them: the rule before "n > 0" */
    bool small = false;        /* whole particles that fit the small-batch grid */
    bool path_carry = false;   /* whole legs and a wave for every particle */
    uint32_t seg_heavy_resolver = 0, seg_heavy_prio = 0, seg_heavy_rel = 0;
    uint64_t seg_done_words = 0, seg_state_words = 0; /* what the launch needs of the two arrays (0: none) */
};
/* segmentable: false for a traced call, which runs whole */
SegmentPlan plan_segments(const Inputs& in, uint64_t n, uint64_t legs, bool segmentable = true);
/* seg_steps, nseg and the heavy-segment settings of a plan, into a call's arguments */
void apply_segments(const SegmentPlan& p, fksd::SimArgs* a);

/* The normal form: a span of path jobs.  A path is one path job, a job a path job of one leg. */
struct Batch {
    Form form = PATH_JOBS;
    Entry entry = ENTRY_PATH_JOBS;
    const fks_path_job* external = nullptr; /* the caller's path jobs ... */
    std::vector<fks_path_job> converted;    /* ... or the normal form of a path or a job batch, or a staged copy */
    uint64_t num_jobs = 0;                  /* as the caller passed it (refused before anything is read when too large) */
    /* from check_arguments: the sum of n, of num_legs, the longest job's legs, the sum of n x num_legs */
    uint64_t total = 0, legs = 0, max_legs = 0, rows = 0;
    SegmentPlan plan; /* from plan_batch */
    /* a policy roll-out (fks_forward_simulate_policy): a path of max_legs legs whose records carry
     * no targets, with the table and the three outputs of the selection (from_policy) */
    bool policy = false;
    bool has_table = false; /* the caller passed a table (a NULL one is refused) */
    fks_policy_table table{};
    uint32_t* out_choice = nullptr;
    double* out_distance = nullptr;
    uint32_t* out_legs_run = nullptr;

    const fks_path_job* jobs() const { return converted.empty() ? external : converted.data(); }
};
void from_path(Batch* b, Entry entry, const double* starts, uint64_t n, const double* waypoints, uint64_t num_legs,
               uint64_t num_targets, uint64_t first_particle_id, int32_t allow_contacts, double* out_positions,
               uint8_t* out_collided, uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags);
void from_policy(Batch* b, Entry entry, const double* starts, uint64_t n, const fks_policy_table* table, uint64_t max_legs,
                 uint64_t first_particle_id, int32_t allow_contacts, double* out_positions, uint8_t* out_collided,
                 uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags, uint32_t* out_choice,
                 double* out_distance, uint32_t* out_legs_run);
void from_jobs(Batch* b, const fks_job* jobs, uint64_t num_jobs);
void from_path_jobs(Batch* b, const fks_path_job* jobs, uint64_t num_jobs);
/* a one-leg path job as the job it came from */
fks_job as_job(const fks_path_job& p);

/* What an entry refuses before anything is staged or counted: FKS_OK, or the status with its
 * text in *why.  Fills the batch's sums. */
fks_status check_arguments(Batch* b, bool individual_jacobians, std::string* why);
/* ... and what depends on the context's schedule: the segment plan and the 2^31 bound of a
 * particle's ticket space.  check_arguments, then this. */
fks_status plan_batch(const Inputs& in, Batch* b, std::string* why);

/* the records of a planned batch */
struct RecordPlan {
    size_t records = 0;         /* SimArgs-sized units of the upload: the records, then job_first and leg_first,
                                   then a roll-out's PolicyArgs */
    size_t policy_record = 0;   /* the unit that holds a roll-out's PolicyArgs (0: not a roll-out) */
    uint64_t call_advance = 0;  /* what the call adds to the call index ... */
    uint64_t particles = 0;     /* ... and to last.particles (a roll-out: 0, its kernel counts the pairs it simulates) */
    bool launch = false;        /* false: every job is empty, nothing is uploaded or launched */
};
RecordPlan plan_records(const Batch& b);
/* Writes the upload into h_records (plan_records(b).records units): one record per (job, leg),
 * job-major, then job_first[num_jobs + 1] and leg_first[num_jobs + 1], then a roll-out's
 * PolicyArgs (unit plan_records(b).policy_record).  d_records is where the upload will lie on the
 * device, seg_state / seg_done the batch's arrays (null where the plan needs none). */
void build_records(const Inputs& in, const Batch& b, double* seg_state, uint32_t* seg_done, const fksd::SimArgs* d_records,
                   fksd::SimArgs* h_records);

/* The plan of a clustering call (fks_cluster_configs and its device entries): the groups' offsets
 * checked, the prefix of their n x n matrices, and what the device call needs of its workspace.
 * group_begin is read only when it is non-NULL and num_groups > 0; no other pointer is read. */
struct ClusterPlan {
    uint64_t num_groups = 0;
    uint64_t total = 0;        /* N: configurations in all groups (group_begin[G] - group_begin[0] counted from 0) */
    uint64_t largest = 0;      /* the largest group */
    bool labelled = false;     /* labels or counts are asked for */
    bool launch = false;       /* false: nothing to compute (no group, or only empty ones and no counts) */
    std::vector<uint64_t> mat_begin; /* [G + 1]: group g's matrix at mat_begin[g] doubles; mat_begin[G] = sum of n^2 */
    uint64_t work_words = 0;   /* doubles of the device's HBM link workspace (0: every labelled group's links fit LDS) */
};
constexpr uint64_t kMaxClusterMatrixWords = 1ull << 27;
constexpr uint64_t kMaxClusterConfigs = 1ull << 31;
/* groups of at most this many configurations keep their working link matrix in LDS (fks_kernels.hip) */
constexpr uint64_t kClusterLdsGroup = 64;
fks_status plan_cluster(ClusterPlan* p, const double* configs, const uint64_t* group_begin, uint64_t num_groups, double threshold,
                        const void* out_distances, const void* out_labels, const void* out_num_clusters, std::string* why);

/* The plan of a summary call (fks_summarize_clusters and its device entries): the groups' offsets
 * checked and the widths of the device call's workspace.  group_begin is read only when it is
 * non-NULL and num_groups > 0, *out only when it is non-NULL; no other pointer is read. */
struct SummaryPlan {
    uint64_t num_groups = 0;
    uint64_t total = 0;        /* N = group_begin[G] */
    uint64_t first = 0;        /* group_begin[0]: rows below it belong to no group */
    bool launch = false;       /* false: no group */
    uint32_t width = 0;        /* W */
    uint32_t var_width = 0;    /* Wv: W (linked), 3 (SE(2)), 6 (SE(3)) */
    uint32_t piece_width = 0;  /* doubles of a member's terms in the workspace (fksd::summary_piece_width) */
    uint64_t work_words = 0;   /* doubles of the device's workspace: N x (piece_width + W) */
};
fks_status plan_summary(SummaryPlan* p, int32_t robot_type, uint32_t width, const double* configs, const uint64_t* group_begin,
                        uint64_t num_groups, const uint32_t* labels, const double* targets, double reached_distance,
                        const fks_cluster_summary* out, std::string* why);

/* The plan of a state selection (fks_select_states and its device entries): every refusal, and the
 * decomposition of the device's search.  *table and *out are read when non-NULL; no pointer inside
 * them or `queries` is dereferenced.
 *
 * The rule.  A workgroup of the search takes one tile of queries against one chunk of states.  A
 * tile holds kSelectTile = 8 queries (the last tile of a call fewer), so tiles = ceil(J / 8).  The
 * states are cut into `chunks` equal chunks of chunk_states, a multiple of kSelectThreads = 256:
 * as many chunks as bring tiles x chunks to kSelectGroupsPerCu = 4 workgroups per compute unit, and
 * never more than there are blocks of 256 states, so that every chunk holds a state:
 *     wanted       = ceil(4 x compute_units / tiles)              (1 when the tiles alone fill the device)
 *     chunk_states = 256 x ceil(ceil(S / min(wanted, ceil(S / 256))) / 256)
 *     chunks       = ceil(S / chunk_states)
 * A table of at most 256 states, or a call of at least 32 x compute_units queries, is searched in
 * one chunk.  The result does not depend on the rule: partial results are reduced by (smaller d,
 * then smaller i), which is associative and is the ascending scan's answer for any cut.  The
 * workspace holds one partial (fksd::SelectPartial) per (query, chunk). */
constexpr uint64_t kMaxSelectQueries = 1ull << 20;
constexpr uint64_t kMaxSelectParticles = 65536;
constexpr uint64_t kMaxSelectStarts = 1ull << 31; /* J x P */
constexpr uint64_t kSelectGroupsPerCu = 4;
struct SelectPlan {
    uint64_t num_queries = 0; /* J */
    uint64_t num_states = 0;  /* S */
    uint32_t width = 0;       /* W */
    uint32_t particles = 0;   /* P */
    bool launch = false;      /* false: J == 0 */
    bool draw = false;        /* starts or source is asked for */
    uint32_t tile = 0;          /* queries per workgroup */
    uint64_t tiles = 0;         /* ceil(J / tile) */
    uint64_t chunk_states = 0;  /* states per chunk, a multiple of 256 */
    uint64_t chunks = 0;        /* chunks per query */
    uint64_t groups = 0;        /* tiles x chunks: the search's grid */
    uint64_t work_partials = 0; /* J x chunks */
};
fks_status plan_select(SelectPlan* p, uint32_t width, int32_t compute_units, const fks_state_table* table, const double* queries,
                       uint64_t num_queries, uint32_t num_particles, const fks_state_selection* out, std::string* why);

}  // namespace fks_batch

#endif
