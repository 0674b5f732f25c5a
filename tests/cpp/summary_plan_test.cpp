/*
 * summary_plan_test.cpp — the host-side plan of a summary call (fks_batch::plan_summary) and the
 * host twin fks_summarize_clusters without a GPU: every refusal's status and text, the widths and
 * the workspace of a plan, and the twin on hand cases (a one-dof prismatic robot of weight 1, whose
 * arithmetic is exact; an SE(2) robot across the angle's seam; an SE(3) pose pair) on exactly-sized
 * heap buffers, so the sanitizer watches their ends: out-of-range labels at a group's first and
 * last row among them.  Links only the HIP-free units fks_batch.cpp, fks_summary.cpp,
 * fks_policy_select.cpp and fks_robot.cpp.
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

static bool refused(const uint64_t* begin, uint64_t G, const void* configs, const void* labels, const void* targets, double reach,
                    const fks_cluster_summary* out, const char* text) {
    SummaryPlan p;
    std::string why;
    const fks_status st = plan_summary(&p, FKS_ROBOT_LINKED, 3, static_cast<const double*>(configs), begin, G,
                                       static_cast<const uint32_t*>(labels), static_cast<const double*>(targets), reach, out, &why);
    return st == FKS_ERR_INVALID_ARGUMENT && why.find(text) != std::string::npos;
}

static void test_plan() {
    double q[4]; /* never dereferenced */
    uint32_t l[4];
    fks_cluster_summary count_only;
    std::memset(&count_only, 0, sizeof(count_only));
    count_only.count = l;
    fks_cluster_summary with_reached = count_only;
    with_reached.reached = l;
    fks_cluster_summary nothing;
    std::memset(&nothing, 0, sizeof(nothing));
    const uint64_t ok[4] = {2, 5, 5, 70};
    SummaryPlan p;
    std::string why;
    CHECK(plan_summary(&p, FKS_ROBOT_LINKED, 3, q, ok, 3, l, nullptr, 0.0, &count_only, &why) == FKS_OK);
    CHECK(p.num_groups == 3 && p.total == 70 && p.first == 2 && p.launch && p.width == 3 && p.var_width == 3 && p.piece_width == 6);
    CHECK(p.work_words == 70 * (6 + 3));
    CHECK(plan_summary(&p, FKS_ROBOT_LINKED, 1, q, ok, 3, l, nullptr, 0.0, &count_only, &why) == FKS_OK && p.piece_width == 2);
    CHECK(plan_summary(&p, FKS_ROBOT_SE2, 3, q, ok, 3, l, q, 1.0, &with_reached, &why) == FKS_OK);
    CHECK(p.var_width == 3 && p.piece_width == 4 && p.work_words == 70 * (4 + 3));
    CHECK(plan_summary(&p, FKS_ROBOT_SE3, 12, q, ok, 3, l, nullptr, kNaN, &count_only, &why) == FKS_OK); /* no targets: the reach is not read */
    CHECK(p.var_width == 6 && p.piece_width == 23 && p.work_words == 70 * (23 + 12));
    /* every index a kernel uses in a member's row lies inside the row: the sin and cos slots of every
     * circular component, the SE(3) products and sums, the squares and the squared distance */
    for (uint32_t W = 1; W <= 64; ++W) {
        CHECK(fksd::summary_row_end(FKS_ROBOT_LINKED, W) <= fksd::summary_piece_width(FKS_ROBOT_LINKED, W));
        for (uint32_t k = 0; k < W; ++k) CHECK(fksd::summary_term_slot(FKS_ROBOT_LINKED, k) + 1 < fksd::summary_piece_width(FKS_ROBOT_LINKED, W));
        CHECK(W + 1 <= fksd::summary_piece_width(FKS_ROBOT_LINKED, W));
    }
    CHECK(fksd::summary_term_slot(FKS_ROBOT_SE2, 2) + 1 < fksd::summary_piece_width(FKS_ROBOT_SE2, 3));
    CHECK(fksd::summary_row_end(FKS_ROBOT_SE2, 3) == 4 && fksd::summary_piece_width(FKS_ROBOT_SE2, 3) == 4);
    CHECK(fksd::summary_row_end(FKS_ROBOT_SE3, 12) == 23 && fksd::summary_piece_width(FKS_ROBOT_SE3, 12) == 23);
    /* no group, with or without offsets; empty groups */
    CHECK(plan_summary(&p, FKS_ROBOT_LINKED, 3, nullptr, nullptr, 0, nullptr, nullptr, 0.0, &count_only, &why) == FKS_OK && !p.launch);
    const uint64_t zero[3] = {0, 0, 0};
    CHECK(plan_summary(&p, FKS_ROBOT_LINKED, 3, nullptr, zero, 2, nullptr, nullptr, 0.0, &count_only, &why) == FKS_OK && p.launch &&
          p.total == 0 && p.work_words == 0);
    /* the bounds themselves pass */
    const uint64_t full[2] = {0, FKS_MAX_CLUSTER_GROUP};
    CHECK(plan_summary(&p, FKS_ROBOT_LINKED, 3, q, full, 1, l, nullptr, 0.0, &count_only, &why) == FKS_OK);
    const uint64_t far[3] = {(1ull << 31) - 1, (1ull << 31) - 1, 1ull << 31};
    CHECK(plan_summary(&p, FKS_ROBOT_LINKED, 3, q, far, 2, l, nullptr, 0.0, &count_only, &why) == FKS_OK && p.total == (1ull << 31));
    CHECK(plan_summary(&p, FKS_ROBOT_LINKED, 3, q, ok, 3, l, q, kInf, &with_reached, &why) == FKS_OK);
    /* refusals */
    CHECK(refused(ok, 3, q, l, nullptr, 0.0, nullptr, "null summary"));
    CHECK(refused(ok, 3, q, l, nullptr, 0.0, &nothing, "every pointer of the summary is NULL"));
    CHECK(refused(ok, 3, q, nullptr, nullptr, 0.0, &count_only, "null labels"));
    CHECK(refused(ok, 3, nullptr, l, nullptr, 0.0, &count_only, "null configs"));
    CHECK(refused(ok, 3, q, l, nullptr, 1.0, &with_reached, "reached is asked for without targets"));
    CHECK(refused(ok, 3, q, l, q, 1.0, &count_only, "targets are given without reached"));
    CHECK(refused(ok, 3, q, l, q, kNaN, &with_reached, "reached_distance is NaN"));
    CHECK(refused(nullptr, 3, q, l, nullptr, 0.0, &count_only, "null group_begin"));
    const uint64_t back[4] = {0, 5, 4, 9};
    CHECK(refused(back, 3, q, l, nullptr, 0.0, &count_only, "ascending"));
    const uint64_t over[3] = {0, 2, 2 + FKS_MAX_CLUSTER_GROUP + 1};
    CHECK(refused(over, 2, q, l, nullptr, 0.0, &count_only, "FKS_MAX_CLUSTER_GROUP"));
    const uint64_t many[2] = {0, (1ull << 31) + 1};
    CHECK(refused(many, 1, q, l, nullptr, 0.0, &count_only, "2^31"));
    CHECK(refused(ok, 1ull << 31, q, l, nullptr, 0.0, &count_only, "groups"));
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

/* every output of one call on exactly-sized heap buffers */
struct Outputs {
    std::vector<uint32_t> order, count, begin, reached;
    std::vector<double> members, expectation, variances, variance;
    fks_cluster_summary s;
    Outputs(size_t N, size_t W, size_t Wv, bool with_reached)
        : order(N, 99u), count(N, 99u), begin(N, 99u), reached(with_reached ? N : 0, 99u), members(N * W, -1.0),
          expectation(N * W, -1.0), variances(N * Wv, -1.0), variance(N, -1.0) {
        s.order = order.data();
        s.members = members.data();
        s.count = count.data();
        s.begin = begin.data();
        s.expectation = expectation.data();
        s.variances = variances.data();
        s.variance = variance.data();
        s.reached = with_reached ? reached.data() : nullptr;
    }
};
typedef std::vector<uint32_t> L;
typedef std::vector<double> D;

static void test_twin() {
    fks_joint_desc joint;
    fks_dof_controller ctrl;
    const double one = 1.0;
    const fks_robot_desc r = slider(&joint, &ctrl, &one);
    {
        /* labels [2, 0, 2, 9, 0]: 9 is out of range; the target 2 with the strict reach 1 */
        const D q = {1.0, 10.0, 3.0, 7.0, 20.0};
        const L lab = {2, 0, 2, 9, 0};
        const uint64_t begin[2] = {0, 5};
        const double target = 2.0;
        Outputs o(5, 1, 1, true);
        CHECK(fks_summarize_clusters(&r, q.data(), begin, 1, lab.data(), &target, 1.0, &o.s) == FKS_OK);
        CHECK((o.order == L{1, 4, 0, 2, 3}) && (o.members == D{10.0, 20.0, 1.0, 3.0, 7.0}));
        CHECK((o.count == L{2, 0, 2, 0, 0}) && (o.begin == L{0, 2, 2, 4, 4}) && (o.reached == L{0, 0, 0, 0, 0}));
        CHECK((o.expectation == D{15.0, 0.0, 2.0, 0.0, 0.0}) && (o.variances == D{25.0, 0.0, 1.0, 0.0, 0.0}) && o.variances == o.variance);
        CHECK(!std::signbit(o.expectation[1]) && !std::signbit(o.variance[3]));
        Outputs p(5, 1, 1, true);
        CHECK(fks_summarize_clusters(&r, q.data(), begin, 1, lab.data(), &target, std::nextafter(1.0, 2.0), &p.s) == FKS_OK);
        CHECK((p.reached == L{0, 0, 2, 0, 0}));
    }
    {
        /* three groups from offset 1: out-of-range labels at the first and the last row of a group, an
         * empty group, rows below the first offset untouched; each output alone */
        const D q = {9.0, 4.0, 6.0, 8.0, 1.0, 2.0};
        const L lab = {0, 0xFFFFFFFFu, 0, 3, 0, 2};
        const uint64_t begin[4] = {1, 4, 4, 6};
        Outputs o(6, 1, 1, false);
        CHECK(fks_summarize_clusters(&r, q.data(), begin, 3, lab.data(), nullptr, 0.0, &o.s) == FKS_OK);
        CHECK((o.order == L{99, 2, 1, 3, 4, 5}) && (o.members == D{-1.0, 6.0, 4.0, 8.0, 1.0, 2.0}));
        CHECK((o.count == L{99, 1, 0, 0, 1, 0}) && (o.begin == L{99, 1, 2, 2, 4, 5}));
        CHECK((o.expectation == D{-1.0, 6.0, 0.0, 0.0, 1.0, 0.0}) && (o.variance == D{-1.0, 0.0, 0.0, 0.0, 0.0, 0.0}));
        std::vector<uint32_t> only(6, 99u);
        fks_cluster_summary s;
        std::memset(&s, 0, sizeof(s));
        s.begin = only.data();
        CHECK(fks_summarize_clusters(&r, q.data(), begin, 3, lab.data(), nullptr, 0.0, &s) == FKS_OK && (only == L{99, 1, 2, 2, 4, 5}));
        std::vector<double> var(6, -1.0);
        std::memset(&s, 0, sizeof(s));
        s.variance = var.data();
        CHECK(fks_summarize_clusters(&r, q.data(), begin, 3, lab.data(), nullptr, 0.0, &s) == FKS_OK && var[0] == -1.0 && var[1] == 0.0);
    }
    {
        /* a full group of 256 in one cluster and one of all singletons in descending labels */
        D q(512);
        L lab(512);
        for (size_t i = 0; i < 256; ++i) {
            q[i] = (double)i;
            lab[i] = 0;
            q[256 + i] = (double)i;
            lab[256 + i] = (uint32_t)(255 - i);
        }
        const uint64_t begin[3] = {0, 256, 512};
        Outputs o(512, 1, 1, false);
        CHECK(fks_summarize_clusters(&r, q.data(), begin, 2, lab.data(), nullptr, 0.0, &o.s) == FKS_OK);
        CHECK(o.count[0] == 256 && o.count[1] == 0 && o.begin[1] == 256 && o.begin[255] == 256 && o.expectation[0] == 127.5);
        CHECK(o.variances[0] == (256.0 * 256.0 - 1.0) / 12.0); /* every term and partial sum is exact */
        CHECK(o.order[256] == 511 && o.order[511] == 256 && o.count[256] == 1 && o.begin[300] == 300 && o.expectation[256] == 255.0);
        const uint64_t b257[2] = {0, 257};
        CHECK(fks_summarize_clusters(&r, q.data(), b257, 1, lab.data(), nullptr, 0.0, &o.s) == FKS_ERR_INVALID_ARGUMENT);
    }
    /* refusals of the entry itself */
    {
        const D q = {1.0};
        const L lab = {0};
        const uint64_t begin[2] = {0, 1};
        Outputs o(1, 1, 1, false);
        CHECK(fks_summarize_clusters(nullptr, q.data(), begin, 1, lab.data(), nullptr, 0.0, &o.s) == FKS_ERR_INVALID_ARGUMENT);
        fks_robot_desc bad = r;
        bad.num_dofs = 2;
        CHECK(fks_summarize_clusters(&bad, q.data(), begin, 1, lab.data(), nullptr, 0.0, &o.s) == FKS_ERR_INVALID_ARGUMENT);
        CHECK(fks_summarize_clusters(&r, q.data(), begin, 1, lab.data(), nullptr, 0.0, nullptr) == FKS_ERR_INVALID_ARGUMENT);
        CHECK(fks_summarize_clusters(&r, q.data(), begin, 1, nullptr, nullptr, 0.0, &o.s) == FKS_ERR_INVALID_ARGUMENT);
        CHECK(o.count[0] == 99u);
        CHECK(fks_summarize_clusters(&r, nullptr, nullptr, 0, nullptr, nullptr, 0.0, &o.s) == FKS_OK);
    }
    const double pi = 3.14159265358979323846;
    {
        /* SE(2): the circular mean across the seam and the wrapped difference */
        fks_dof_controller ctrl3[3];
        std::memset(ctrl3, 0, sizeof(ctrl3));
        const double w2[2] = {1.0, 0.5};
        fks_robot_desc se2;
        std::memset(&se2, 0, sizeof(se2));
        se2.robot_type = FKS_ROBOT_SE2;
        se2.num_dofs = 3;
        se2.controllers = ctrl3;
        se2.distance_weights = w2;
        const D q = {1.0, 2.0, pi - 0.25, 3.0, 2.0, -pi + 0.25 + 2 * pi};
        const L lab = {0, 0};
        const uint64_t begin[2] = {0, 2};
        Outputs o(2, 3, 3, false);
        CHECK(fks_summarize_clusters(&se2, q.data(), begin, 1, lab.data(), nullptr, 0.0, &o.s) == FKS_OK);
        CHECK(o.expectation[0] == 2.0 && o.expectation[1] == 2.0 && std::fabs(std::fabs(o.expectation[2]) - pi) < 1e-15);
        CHECK(o.variances[0] == 1.0 && o.variances[1] == 0.0 && std::fabs(o.variances[2] - 0.0625) < 1e-14);
        CHECK(std::fabs(o.variance[0] - (1.0 + 0.5 * 0.25) * (1.0 + 0.5 * 0.25)) < 1e-14);
    }
    {
        /* SE(3): two poses a quarter turn apart about z; the mean is the eighth turn between them, and -R's
         * quaternion sign plays no part */
        fks_dof_controller ctrl6[6];
        std::memset(ctrl6, 0, sizeof(ctrl6));
        const double w2[2] = {1.0, 1.0};
        fks_robot_desc se3;
        std::memset(&se3, 0, sizeof(se3));
        se3.robot_type = FKS_ROBOT_SE3;
        se3.num_dofs = 6;
        se3.controllers = ctrl6;
        se3.distance_weights = w2;
        const D q = {1, 0, 0, 0.0, 0, 1, 0, 0.0, 0, 0, 1, 0.0, 0, -1, 0, 2.0, 1, 0, 0, 0.0, 0, 0, 1, 4.0};
        const L lab = {0, 0};
        const uint64_t begin[2] = {0, 2};
        Outputs o(2, 12, 6, false);
        CHECK(fks_summarize_clusters(&se3, q.data(), begin, 1, lab.data(), nullptr, 0.0, &o.s) == FKS_OK);
        const double h = std::sqrt(0.5);
        CHECK(std::fabs(o.expectation[0] - h) < 1e-15 && std::fabs(o.expectation[1] + h) < 1e-15 && std::fabs(o.expectation[4] - h) < 1e-15);
        CHECK(std::fabs(o.expectation[10] - 1.0) < 1e-15 && o.expectation[3] == 1.0 && o.expectation[7] == 0.0 && o.expectation[11] == 2.0);
        CHECK(std::fabs(o.variances[5] - (pi / 4) * (pi / 4)) < 1e-14 && std::fabs(o.variances[3]) < 1e-28 && std::fabs(o.variances[4]) < 1e-28);
        for (size_t k = 12; k < 24; ++k) CHECK(o.expectation[k] == 0.0);
    }
}

int main() {
    test_plan();
    test_twin();
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("summary plan test ok\n");
    return 0;
}
