/*
 * policy_plan_test.cpp — the host-side plan of a policy roll-out (fks_forward_simulate_policy)
 * without a GPU: every refusal's status and text, the records (one per leg, no targets), the
 * staging of the PolicyArgs record behind them, and fks_policy_select on hand cases.  Small host
 * arrays stand in for the device buffers (the planner offsets and stores the pointers, it never
 * dereferences them).  Links only the HIP-free units fks_batch.cpp and fks_policy_select.cpp.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "fks_batch.h"

using namespace fks_batch;
using fksd::PolicyArgs;
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
const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();

static Inputs inputs(uint32_t segment_steps = 0) {
    Inputs in;
    in.seed = kSeed;
    in.call_index = kCall;
    in.T = 20;
    in.segment_steps = segment_steps;
    in.grid_waves = 4;
    in.small_grid_waves = 2;
    in.W = W;
    in.seg_stride = 7;
    std::memset(&in.base, 0, sizeof(in.base));
    in.base.dt = 0.1;
    return in;
}

/* stand-ins for device buffers */
static double g_starts[64], g_keys[64], g_targets[64], g_out[512], g_dist[128], g_state[1024];
static uint32_t g_flags[16], g_choice[128], g_legs[16], g_res[128], g_done[16];
static uint8_t g_coll[128];

static fks_policy_table table(uint64_t M = 5) {
    fks_policy_table t;
    std::memset(&t, 0, sizeof(t));
    t.keys = g_keys;
    t.targets = g_targets;
    t.flags = g_flags;
    t.num_entries = M;
    t.terminal_distance = 0.5;
    t.max_distance = kInf;
    return t;
}

static void roll_out(Batch* b, Entry entry, uint64_t n, const fks_policy_table* t, uint64_t legs, uint32_t* out_choice = g_choice,
                     double* out_positions = g_out, const double* starts = g_starts) {
    from_policy(b, entry, starts, n, t, legs, 11, 1, out_positions, g_coll, nullptr, g_res, nullptr, out_choice, g_dist, g_legs);
}

static void refused(Entry entry, uint64_t n, const fks_policy_table* t, uint64_t legs, fks_status want, const char* text,
                    bool individual = false, uint32_t* out_choice = g_choice, double* out_positions = g_out,
                    const double* starts = g_starts, uint32_t segment_steps = 0) {
    Batch b;
    roll_out(&b, entry, n, t, legs, out_choice, out_positions, starts);
    std::string why;
    const Inputs in = inputs(segment_steps);
    fks_status st = check_arguments(&b, individual, &why);
    if (st == FKS_OK) st = plan_batch(in, &b, &why);
    if (st != want || why != text) {
        std::fprintf(stderr, "refusal: got %d \"%s\", want %d \"%s\"\n", (int)st, why.c_str(), (int)want, text);
        ++g_failures;
    }
}

static void test_refusals() {
    const fks_policy_table ok = table();
    for (Entry e : {ENTRY_POLICY_DEVICE, ENTRY_POLICY_HOST}) {
        const bool host = e == ENTRY_POLICY_HOST;
        refused(e, 4, &ok, 0, FKS_ERR_INVALID_ARGUMENT, "a roll-out needs at least one leg (max_legs)");
        refused(e, 4, &ok, 3, FKS_ERR_UNSUPPORTED,
                "no policy kernel with individual Jacobians (fks_set_individual_jacobians): chain plain calls", true);
        refused(e, 4, nullptr, 3, FKS_ERR_INVALID_ARGUMENT, "null policy table");
        fks_policy_table t = table(0);
        refused(e, 4, &t, 3, FKS_ERR_INVALID_ARGUMENT, "a policy table needs at least one entry");
        t = table((1ull << 30) + 1);
        refused(e, 4, &t, 3, FKS_ERR_INVALID_ARGUMENT, "at most 2^30 policy entries");
        t = table();
        t.keys = nullptr;
        refused(e, 0, &t, 3, FKS_ERR_INVALID_ARGUMENT, "null policy keys or targets"); /* also without particles */
        t = table();
        t.targets = nullptr;
        refused(e, 4, &t, 3, FKS_ERR_INVALID_ARGUMENT, "null policy keys or targets");
        t = table();
        t.terminal_distance = kNaN;
        refused(e, 4, &t, 3, FKS_ERR_INVALID_ARGUMENT, "terminal_distance or max_distance is NaN");
        t = table();
        t.max_distance = kNaN;
        refused(e, 4, &t, 3, FKS_ERR_INVALID_ARGUMENT, "terminal_distance or max_distance is NaN");
        const char* null_text = host ? "null host buffer (starts, out_positions or out_choice)"
                                     : "null device buffer (starts, out_positions or out_choice)";
        refused(e, 4, &ok, 3, FKS_ERR_INVALID_ARGUMENT, null_text, false, nullptr);
        refused(e, 4, &ok, 3, FKS_ERR_INVALID_ARGUMENT, null_text, false, g_choice, nullptr);
        refused(e, 4, &ok, 3, FKS_ERR_INVALID_ARGUMENT, null_text, false, g_choice, g_out, nullptr);
        /* legs x segments per leg: 20 steps in segments of 1, also for an empty batch (the path's rule) */
        const uint64_t too_many = (1ull << 31) / 20 + 1;
        refused(e, 4, &ok, too_many, FKS_ERR_INVALID_ARGUMENT, "legs x segments per leg must stay below 2^31", false, g_choice, g_out,
                g_starts, 1);
        refused(e, 0, &ok, too_many, FKS_ERR_INVALID_ARGUMENT, "legs x segments per leg must stay below 2^31", false, g_choice, g_out,
                g_starts, 1);
        refused(e, 4, &ok, 1ull << 31, FKS_ERR_INVALID_ARGUMENT, host ? "roll-out too large" : "legs x segments per leg must stay below 2^31");
        refused(e, 1ull << 32, &ok, 3, FKS_ERR_INVALID_ARGUMENT, host ? "roll-out too large" : "at most 2^32-1 particles per call");
    }
    /* accepted: no flags, no optional outputs, no particles with null buffers */
    Batch b;
    fks_policy_table t = table(1);
    t.flags = nullptr;
    from_policy(&b, ENTRY_POLICY_DEVICE, nullptr, 0, &t, 2, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    std::string why;
    CHECK(check_arguments(&b, false, &why) == FKS_OK);
    CHECK(plan_batch(inputs(), &b, &why) == FKS_OK);
    const RecordPlan rp = plan_records(b);
    CHECK(!rp.launch && rp.call_advance == 2 && rp.particles == 0);
}

static void test_records(uint32_t segment_steps, uint64_t n) {
    const uint64_t K = 3;
    const Inputs in = inputs(segment_steps);
    Batch b;
    const fks_policy_table t = table();
    roll_out(&b, ENTRY_POLICY_DEVICE, n, &t, K);
    std::string why;
    CHECK(check_arguments(&b, false, &why) == FKS_OK);
    CHECK(plan_batch(in, &b, &why) == FKS_OK);
    CHECK(b.policy && b.form == PATH && b.total == n && b.legs == K && b.max_legs == K && b.rows == n * K);
    const RecordPlan rp = plan_records(b);
    /* K records, one unit of prefix arrays (a single job), then the PolicyArgs */
    CHECK(rp.records == K + 2 && rp.policy_record == K + 1);
    CHECK(rp.call_advance == K && rp.particles == 0 && rp.launch);
    /* the kernel choice and the schedule are a path's over n */
    const SegmentPlan path_plan = plan_segments(in, n, K);
    CHECK(b.plan.small == path_plan.small && b.plan.nseg == path_plan.nseg && b.plan.path_carry == path_plan.path_carry);
    CHECK(b.plan.seg_done_words == n); /* K > 1: a stopped particle retires its ticket space there */
    std::vector<SimArgs> h(rp.records), d(rp.records);
    std::memset(h.data(), 0xab, h.size() * sizeof(SimArgs));
    build_records(in, b, b.plan.seg_state_words ? g_state : nullptr, g_done, d.data(), h.data());
    for (uint64_t k = 0; k < K; ++k) {
        const SimArgs& r = h[k];
        const uint64_t key = splitmix64(kSeed ^ splitmix64(kCall + k));
        CHECK(((uint64_t)r.key0 | ((uint64_t)r.key1 << 32)) == key);
        CHECK(r.targets == nullptr && r.num_targets == n); /* no targets: chosen on the device, one per particle */
        CHECK(r.n == n && r.first_pid == 11 && r.allow_contacts == 1 && r.path_legs == K);
        CHECK(r.starts == (k == 0 ? g_starts : g_out + (k - 1) * n * W));
        CHECK(r.out_q == g_out + k * n * W && r.out_collided == g_coll + k * n && r.out_resolver == g_res + k * n);
        CHECK(r.out_micro == nullptr && r.out_err == nullptr);
        CHECK(r.seg_done == g_done && r.nseg == b.plan.nseg);
    }
    PolicyArgs p;
    std::memcpy(&p, h.data() + rp.policy_record, sizeof(p));
    CHECK(p.keys == g_keys && p.targets == g_targets && p.flags == g_flags && p.num_entries == 5);
    CHECK(p.terminal_distance == 0.5 && p.max_distance == kInf);
    CHECK(p.out_choice == g_choice && p.out_distance == g_dist && p.out_legs_run == g_legs);
}

/* fks_policy_select on hand cases: an SE(2) robot and a two-joint arm with one continuous dof */
static void test_select() {
    fks_dof_controller ctrl[3];
    std::memset(ctrl, 0, sizeof(ctrl));
    const double w2[2] = {1.0, 0.5};
    fks_robot_desc se2;
    std::memset(&se2, 0, sizeof(se2));
    se2.robot_type = FKS_ROBOT_SE2;
    se2.num_dofs = 3;
    se2.controllers = ctrl;
    se2.distance_weights = w2;
    /* keys: A (3, 4 away in xy), its duplicate, B across the angle's seam; then A, C (0.5 away, terminal), a NaN key */
    const double keys[3 * 3] = {4.0, 5.0, 0.0, 4.0, 5.0, 0.0, 1.0, 1.0, -3.0};
    const double tkeys[3 * 3] = {4.0, 5.0, 0.0, 1.0, 1.5, 3.0, kNaN, 0.0, 0.0};
    const uint32_t flags[3] = {0, FKS_POLICY_ENTRY_TERMINAL, FKS_POLICY_ENTRY_TERMINAL};
    fks_policy_table t;
    std::memset(&t, 0, sizeof(t));
    t.keys = keys;
    t.targets = keys;
    t.num_entries = 2;
    t.max_distance = kInf;
    const double q[2 * 3] = {1.0, 1.0, 3.0, 1.0, 1.0, 3.0 + 4 * 3.14159265358979323846};
    uint32_t choice[2];
    double dist[2];
    CHECK(fks_policy_select(&se2, &t, q, 2, choice, dist) == FKS_OK);
    CHECK(choice[0] == 0 && dist[0] == 5.0 + 0.5 * 3.0); /* the duplicate at index 1 never wins */
    t.num_entries = 3;
    CHECK(fks_policy_select(&se2, &t, q, 2, choice, dist) == FKS_OK);
    CHECK(choice[0] == 2 && std::fabs(dist[0] - 0.5 * (2 * 3.14159265358979323846 - 6.0)) < 1e-15); /* across the seam */
    CHECK(choice[1] == 2 && std::fabs(dist[1] - dist[0]) < 1e-14);                                   /* two turns out: reset first */
    t.keys = tkeys; /* the NaN key never wins; entry 1 is 0.5 away and terminal */
    t.num_entries = 3;
    t.flags = flags;
    t.terminal_distance = 0.5;
    CHECK(fks_policy_select(&se2, &t, q, 1, choice, dist) == FKS_OK);
    CHECK(choice[0] == 1 && dist[0] == 0.5); /* d == terminal_distance: not arrived */
    t.terminal_distance = 0.75;
    CHECK(fks_policy_select(&se2, &t, q, 1, choice, nullptr) == FKS_OK);
    CHECK(choice[0] == (1u | FKS_POLICY_ARRIVED));
    t.max_distance = 0.5;
    CHECK(fks_policy_select(&se2, &t, q, 1, choice, dist) == FKS_OK);
    CHECK(choice[0] == (1u | FKS_POLICY_ARRIVED)); /* d == max_distance: not lost */
    t.max_distance = 0.25;
    CHECK(fks_policy_select(&se2, &t, q, 1, choice, dist) == FKS_OK);
    CHECK(choice[0] == FKS_POLICY_LOST && dist[0] == 0.5); /* the lost test wins over the terminal test */
    t.keys = tkeys + 6; /* only the NaN key */
    t.num_entries = 1;
    t.max_distance = kInf;
    CHECK(fks_policy_select(&se2, &t, q, 1, choice, dist) == FKS_OK);
    CHECK(choice[0] == FKS_POLICY_LOST && dist[0] == kInf);
    /* refusals */
    t.num_entries = 0;
    CHECK(fks_policy_select(&se2, &t, q, 1, choice, dist) == FKS_ERR_INVALID_ARGUMENT);
    t.num_entries = 1;
    t.max_distance = kNaN;
    CHECK(fks_policy_select(&se2, &t, q, 1, choice, dist) == FKS_ERR_INVALID_ARGUMENT);
    t.max_distance = kInf;
    CHECK(fks_policy_select(&se2, &t, q, 1, nullptr, dist) == FKS_ERR_INVALID_ARGUMENT);
    CHECK(fks_policy_select(nullptr, &t, q, 1, choice, dist) == FKS_ERR_INVALID_ARGUMENT);
    CHECK(fks_policy_select(&se2, nullptr, q, 1, choice, dist) == FKS_ERR_INVALID_ARGUMENT);
    CHECK(fks_policy_select(&se2, &t, nullptr, 0, nullptr, nullptr) == FKS_OK);

    /* a revolute joint limited to [-1, 1] and a continuous one, weights 2 and 1 */
    fks_joint_desc joints[3];
    std::memset(joints, 0, sizeof(joints));
    joints[0].type = FKS_JOINT_REVOLUTE;
    joints[0].limit_lower = -1.0;
    joints[0].limit_upper = 1.0;
    joints[1].type = FKS_JOINT_FIXED;
    joints[2].type = FKS_JOINT_CONTINUOUS;
    const double wl[2] = {2.0, 1.0};
    fks_robot_desc arm;
    std::memset(&arm, 0, sizeof(arm));
    arm.robot_type = FKS_ROBOT_LINKED;
    arm.num_joints = 3;
    arm.num_dofs = 2;
    arm.joints = joints;
    arm.controllers = ctrl;
    arm.distance_weights = wl;
    const double akeys[2 * 2] = {1.5, 0.0, 0.75, 0.0};
    t.keys = akeys;
    t.targets = akeys;
    t.flags = nullptr;
    t.num_entries = 2;
    const double aq[2] = {1.5, 0.0}; /* clamped to 1.0: entry 1 (0.25 x 2) beats entry 0 (0.5 x 2), which the raw value equals */
    CHECK(fks_policy_select(&arm, &t, aq, 1, choice, dist) == FKS_OK);
    CHECK(choice[0] == 1 && dist[0] == 0.5);
}

int main() {
    test_refusals();
    for (uint32_t segment_steps : {0u, 7u})
        for (uint64_t n : {2ull, 3ull, 9ull}) test_records(segment_steps, n);
    test_select();
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("policy plan test ok\n");
    return 0;
}
