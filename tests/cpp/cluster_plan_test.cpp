/*
 * cluster_plan_test.cpp — the host-side plan of a clustering call (fks_batch::plan_cluster) and the
 * host twin fks_cluster_configs without a GPU: every refusal's status and text, the matrices'
 * prefix and the workspace of a plan, and the twin on hand cases (a one-dof prismatic robot of
 * weight 1, whose distances are exact; an SE(2) robot across the angle's seam), with guard words
 * around every output.  fks_policy_select runs once beside it: both stand on fks_host_distance.h.
 * Links only the HIP-free units fks_batch.cpp, fks_cluster.cpp and fks_policy_select.cpp.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "fks_batch.h"

using namespace fks_batch;

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                  \
        }                                                                  \
    } while (0)

const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();

static bool refused(const uint64_t* begin, uint64_t G, double threshold, const void* configs, const void* m, const void* l,
                    const void* c, const char* text) {
    ClusterPlan p;
    std::string why;
    const fks_status st = plan_cluster(&p, static_cast<const double*>(configs), begin, G, threshold, m, l, c, &why);
    return st == FKS_ERR_INVALID_ARGUMENT && why.find(text) != std::string::npos;
}

static void test_plan() {
    double q[4];
    const void* some = q; /* never dereferenced */
    const uint64_t ok[4] = {0, 3, 3, 68};
    ClusterPlan p;
    std::string why;
    CHECK(plan_cluster(&p, q, ok, 3, 1.0, some, some, some, &why) == FKS_OK);
    CHECK(p.num_groups == 3 && p.total == 68 && p.largest == 65 && p.labelled && p.launch);
    CHECK(p.mat_begin.size() == 4 && p.mat_begin[0] == 0 && p.mat_begin[1] == 9 && p.mat_begin[2] == 9 && p.mat_begin[3] == 9 + 65 * 65);
    CHECK(p.work_words == 9 + 65 * 65); /* a labelled group above kClusterLdsGroup: the links lie in HBM */
    CHECK(plan_cluster(&p, q, ok, 3, 1.0, some, nullptr, nullptr, &why) == FKS_OK);
    CHECK(!p.labelled && p.work_words == 0);
    const uint64_t small[3] = {2, 66, 130};
    CHECK(plan_cluster(&p, q, small, 2, -1.0, nullptr, nullptr, some, &why) == FKS_OK);
    CHECK(p.labelled && p.work_words == 0 && p.largest == 64 && p.total == 130 && p.mat_begin[2] == 2 * 64 * 64);
    /* no group, with or without offsets; empty groups */
    CHECK(plan_cluster(&p, nullptr, nullptr, 0, kInf, nullptr, some, nullptr, &why) == FKS_OK && !p.launch && p.num_groups == 0);
    const uint64_t zero[3] = {0, 0, 0};
    CHECK(plan_cluster(&p, nullptr, zero, 2, 0.0, some, some, some, &why) == FKS_OK && p.launch && p.total == 0 && p.mat_begin[2] == 0);
    /* the bounds themselves pass */
    const uint64_t full[2] = {0, FKS_MAX_CLUSTER_GROUP};
    CHECK(plan_cluster(&p, q, full, 1, 1.0, nullptr, some, some, &why) == FKS_OK && p.work_words == 256 * 256);
    const uint64_t wide[2] = {0, 11585};
    CHECK(plan_cluster(&p, q, wide, 1, 1.0, some, nullptr, nullptr, &why) == FKS_OK && p.mat_begin[1] == 11585ull * 11585ull);
    const uint64_t far[3] = {(1ull << 31) - 1, (1ull << 31) - 1, 1ull << 31};
    CHECK(plan_cluster(&p, q, far, 2, 1.0, some, some, some, &why) == FKS_OK && p.total == (1ull << 31));
    /* refusals */
    CHECK(refused(ok, 3, kNaN, q, some, some, some, "NaN"));
    CHECK(refused(ok, 3, 1.0, q, nullptr, nullptr, nullptr, "all NULL"));
    CHECK(refused(nullptr, 3, 1.0, q, some, some, some, "null group_begin"));
    const uint64_t back[4] = {0, 5, 4, 9};
    CHECK(refused(back, 3, 1.0, q, some, some, some, "ascending"));
    CHECK(refused(ok, 3, 1.0, nullptr, some, some, some, "null configs"));
    const uint64_t over[2] = {0, FKS_MAX_CLUSTER_GROUP + 1};
    CHECK(refused(over, 1, 1.0, q, nullptr, some, nullptr, "FKS_MAX_CLUSTER_GROUP"));
    CHECK(refused(over, 1, 1.0, q, some, nullptr, some, "FKS_MAX_CLUSTER_GROUP"));
    CHECK(plan_cluster(&p, q, over, 1, 1.0, some, nullptr, nullptr, &why) == FKS_OK);
    const uint64_t wider[2] = {0, 11586};
    CHECK(refused(wider, 1, 1.0, q, some, nullptr, nullptr, "2^27"));
    const uint64_t two[3] = {0, 8192, 8192 + 8193}; /* 2^26 + (2^26 + ...) */
    CHECK(refused(two, 2, 1.0, q, some, nullptr, nullptr, "2^27"));
    const uint64_t many[2] = {0, (1ull << 31) + 1};
    CHECK(refused(many, 1, 1.0, q, some, nullptr, nullptr, "2^31"));
    CHECK(refused(ok, 1ull << 31, 1.0, q, some, some, some, "groups"));
}

static fks_robot_desc slider(fks_joint_desc* joint, fks_dof_controller* ctrl, const double* weight) {
    std::memset(joint, 0, sizeof(*joint));
    std::memset(ctrl, 0, sizeof(*ctrl));
    joint->type = FKS_JOINT_PRISMATIC;
    joint->limit_lower = -100.0;
    joint->limit_upper = 100.0;
    fks_robot_desc r;
    std::memset(&r, 0, sizeof(r));
    r.robot_type = FKS_ROBOT_LINKED;
    r.num_joints = 1;
    r.num_dofs = 1;
    r.joints = joint;
    r.controllers = ctrl;
    r.distance_weights = weight;
    return r;
}

/* one group on exactly-sized heap outputs (the sanitizer watches their ends) */
static std::vector<uint32_t> labels_of(const fks_robot_desc* robot, const std::vector<double>& pts, int W, double threshold,
                                       uint32_t* count, std::vector<double>* matrix = nullptr) {
    const uint64_t n = pts.size() / (size_t)W;
    const uint64_t begin[2] = {0, n};
    std::vector<uint32_t> labels(n, 99u);
    std::vector<double> m(n * n, -1.0);
    CHECK(fks_cluster_configs(robot, pts.data(), begin, 1, threshold, m.data(), labels.data(), count) == FKS_OK);
    if (matrix) *matrix = m;
    return labels;
}

static void test_twin() {
    fks_joint_desc joint;
    fks_dof_controller ctrl;
    const double one = 1.0;
    const fks_robot_desc r = slider(&joint, &ctrl, &one);
    typedef std::vector<uint32_t> L;
    uint32_t c = 0;
    std::vector<double> m;
    CHECK((labels_of(&r, {0.0, 0.6, 1.2}, 1, 1.0, &c, &m) == L{0, 0, 1}) && c == 2); /* single link would merge all */
    CHECK(m[1] == 0.6 && m[3] == 0.6 && m[2] == 1.2 && m[6] == 1.2 && m[5] == 0.6 && m[0] == 0.0 && m[4] == 0.0 && m[8] == 0.0);
    CHECK(!std::signbit(m[0]) && !std::signbit(m[4]));
    CHECK((labels_of(&r, {0.0, 1.0, 2.0}, 1, 1.0, &c) == L{0, 0, 1}) && c == 2); /* equality merges, the lowest pair first */
    CHECK((labels_of(&r, {2.0, 1.0, 0.0}, 1, 1.0, &c) == L{0, 0, 1}) && c == 2);
    CHECK((labels_of(&r, {0.0, 1.0, 2.0}, 1, std::nextafter(1.0, 0.0), &c) == L{0, 1, 2}) && c == 3);
    CHECK((labels_of(&r, {3.0, 1.0, 3.0, 1.0, 2.0}, 1, 0.0, &c) == L{0, 1, 0, 1, 2}) && c == 3);
    CHECK((labels_of(&r, {3.0, 3.0, 1.0}, 1, -1.0, &c) == L{0, 1, 2}) && c == 3);
    CHECK((labels_of(&r, {3.0, 3.0, 1.0, 50.0}, 1, kInf, &c) == L{0, 0, 0, 0}) && c == 1);
    CHECK((labels_of(&r, {0.0, kNaN, 0.5, kInf}, 1, kInf, &c, &m) == L{0, 1, 0, 2}) && c == 3);
    CHECK(std::isnan(m[1]) && std::isnan(m[4 + 0]) && m[3] == kInf && m[4 + 1] == 0.0);
    CHECK((labels_of(&r, {0.0, 0.5, 10.0, 10.125, 20.0}, 1, 1.0, &c) == L{0, 0, 1, 1, 2}) && c == 3); /* by smallest member */
    CHECK((labels_of(&r, {7.0}, 1, 1.0, &c) == L{0}) && c == 1);
    CHECK(labels_of(&r, {}, 1, 1.0, &c).empty() && c == 0);
    /* several groups, offsets that start past 0, each output alone */
    const std::vector<double> q = {9.0, 0.0, 0.25, 5.0, 5.0, 5.5, 7.0};
    const uint64_t begin[5] = {1, 3, 3, 6, 7};
    std::vector<uint32_t> labels(7, 99u), counts(4, 99u);
    std::vector<double> mats(4 + 0 + 9 + 1, -1.0);
    CHECK(fks_cluster_configs(&r, q.data(), begin, 4, 0.25, mats.data(), nullptr, nullptr) == FKS_OK);
    CHECK(mats[1] == 0.25 && mats[2] == 0.25 && mats[4 + 1] == 0.0 && mats[4 + 2] == 0.5 && mats[4 + 5] == 0.5 && mats[13] == 0.0);
    CHECK(fks_cluster_configs(&r, q.data(), begin, 4, 0.25, nullptr, labels.data(), nullptr) == FKS_OK);
    CHECK((labels == L{99, 0, 0, 0, 0, 1, 0}));
    CHECK(fks_cluster_configs(&r, q.data(), begin, 4, 0.25, nullptr, nullptr, counts.data()) == FKS_OK);
    CHECK((counts == L{1, 0, 2, 1}));
    /* a group of 300 without labels; 257 with */
    std::vector<double> line(300);
    for (size_t i = 0; i < line.size(); ++i) line[i] = (double)i;
    const uint64_t b300[2] = {0, 300};
    std::vector<double> big(300 * 300, -1.0);
    CHECK(fks_cluster_configs(&r, line.data(), b300, 1, 1.0, big.data(), nullptr, nullptr) == FKS_OK);
    CHECK(big[3 * 300 + 299] == 296.0 && big[299 * 300 + 3] == 296.0 && big[299 * 300 + 299] == 0.0);
    const uint64_t b257[2] = {0, 257};
    std::vector<uint32_t> l257(257, 99u);
    CHECK(fks_cluster_configs(&r, line.data(), b257, 1, 1.0, nullptr, l257.data(), nullptr) == FKS_ERR_INVALID_ARGUMENT);
    CHECK(l257[0] == 99u);
    const uint64_t b256[2] = {0, 256};
    CHECK(fks_cluster_configs(&r, line.data(), b256, 1, 1.0, nullptr, l257.data(), &c) == FKS_OK);
    CHECK(c == 128 && l257[0] == 0 && l257[1] == 0 && l257[2] == 1 && l257[255] == 127 && l257[256] == 99u);
    /* refusals of the entry itself */
    CHECK(fks_cluster_configs(nullptr, q.data(), begin, 4, 1.0, nullptr, nullptr, counts.data()) == FKS_ERR_INVALID_ARGUMENT);
    fks_robot_desc bad = r;
    bad.num_dofs = 2;
    CHECK(fks_cluster_configs(&bad, q.data(), begin, 4, 1.0, nullptr, nullptr, counts.data()) == FKS_ERR_INVALID_ARGUMENT);
    CHECK(fks_cluster_configs(&r, q.data(), begin, 4, kNaN, nullptr, nullptr, counts.data()) == FKS_ERR_INVALID_ARGUMENT);
    CHECK(fks_cluster_configs(&r, nullptr, nullptr, 0, 1.0, nullptr, nullptr, counts.data()) == FKS_OK);

    /* SE(2): the wrap is inside the difference, whole turns apart are 0 apart */
    fks_dof_controller ctrl3[3];
    std::memset(ctrl3, 0, sizeof(ctrl3));
    const double w2[2] = {1.0, 0.5};
    fks_robot_desc se2;
    std::memset(&se2, 0, sizeof(se2));
    se2.robot_type = FKS_ROBOT_SE2;
    se2.num_dofs = 3;
    se2.controllers = ctrl3;
    se2.distance_weights = w2;
    const double pi = 3.14159265358979323846;
    CHECK((labels_of(&se2, {1.0, 1.0, 3.0, 1.0, 1.0, -3.0, 1.0, 1.0, 3.0 + 4 * pi, 4.0, 5.0, 3.0}, 3, 0.2, &c, &m) == L{0, 0, 0, 1}) && c == 2);
    CHECK(std::fabs(m[1] - 0.5 * (2 * pi - 6.0)) < 1e-15 && std::fabs(m[2]) < 1e-14 && m[3] == 5.0);
    /* ... and fks_policy_select, on the same header, still selects across the seam */
    fks_policy_table t;
    std::memset(&t, 0, sizeof(t));
    const double keys[6] = {4.0, 5.0, 0.0, 1.0, 1.0, -3.0};
    t.keys = keys;
    t.targets = keys;
    t.num_entries = 2;
    t.max_distance = kInf;
    const double p[3] = {1.0, 1.0, 3.0};
    uint32_t choice = 0;
    double dist = 0.0;
    CHECK(fks_policy_select(&se2, &t, p, 1, &choice, &dist) == FKS_OK);
    CHECK(choice == 1 && dist == m[1]);
}

int main() {
    test_plan();
    test_twin();
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("cluster plan test ok\n");
    return 0;
}
