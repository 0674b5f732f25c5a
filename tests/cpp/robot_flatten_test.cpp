/*
 * robot_flatten_test.cpp — the host half of a robot (csrc/fks_robot.h) without a GPU: the dof
 * numbering, every table fks_set_robot uploads, the constants the skip proofs rest on (the per-dof
 * levers, the per-round radii and links), every refusal's status and text, and the SDF analysis.
 * Links only the HIP-free unit fks_robot.cpp.
 *
 * The robots are built in code from dyadic lengths (and 3-4-5 triangles), so every norm and sum
 * below is exact and the expected values, worked out by hand from the definitions (DESIGN.md §4.5,
 * §4.10), are compared with ==:
 *
 *   reach(j, l)   the origin offsets |t| of the joints on the path from joint j's child link down
 *                 to link l, plus max(|lo|, |hi|) * |axis| for each prismatic joint on that path
 *   lever[k]      revolute / continuous dof k of joint j: the largest reach(j, l) + |p| over the
 *                 points p of the geometries on links l that dof k moves, padded
 *                 x * (1 + 1e-9) + 1e-12; +inf if |axis| != 1 or any point of the robot has w != 1.
 *                 prismatic: |axis|, unpadded (+inf only for a w != 1)
 *   lever_box[k]  the same with |centre| + |half extents| of a geometry's local box for |p|; +inf
 *                 if |axis| != 1 or a geometry that k moves has no box (a w != 1); prismatic:
 *                 lever[k]
 *   round r       points 64 r .. 64 r + 63: their count, the largest |p| padded the same way, and
 *                 their link if they share one and every w == 1, else -1
 *   SE(2), SE(3)  lever 1 + 1e-9 for a translation component, max |p| padded for a rotation one
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <string>
#include <vector>

#include "fks_robot.h"

using fks_robot::Dof;
using fks_robot::Flat;

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                  \
        }                                                                  \
    } while (0)

const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();

/* a description and the arrays it points at */
struct Robot {
    fks_robot_desc d;
    std::vector<fks_joint_desc> joints;
    std::vector<int32_t> geom_link;
    std::vector<uint32_t> offsets{0};
    std::vector<double> points;
    std::vector<int32_t> allowed;
    std::vector<fks_dof_controller> ctrl;
    std::vector<double> weights;

    explicit Robot(int32_t type, int32_t links = 1) {
        std::memset(&d, 0, sizeof(d));
        d.robot_type = type;
        d.num_links = links;
        const double base[12] = {1, 0, 0, 0.5, 0, 1, 0, -2, 0, 0, 1, 0.25};
        std::memcpy(d.base_transform, base, sizeof(base));
    }
    /* a joint whose origin is the translation (ox, oy, oz) */
    void joint(int32_t parent, int32_t child, int32_t type, double ox, double oy, double oz, double ax, double ay, double az,
               double lo = -1.0, double hi = 1.0) {
        fks_joint_desc j;
        std::memset(&j, 0, sizeof(j));
        j.parent_link = parent;
        j.child_link = child;
        j.type = type;
        const double origin[12] = {1, 0, 0, ox, 0, 1, 0, oy, 0, 0, 1, oz};
        std::memcpy(j.origin, origin, sizeof(origin));
        j.axis[0] = ax;
        j.axis[1] = ay;
        j.axis[2] = az;
        j.limit_lower = lo;
        j.limit_upper = hi;
        joints.push_back(j);
    }
    /* a geometry on `link` of the points xyzw (4 doubles each) */
    void geometry(int32_t link, std::initializer_list<double> xyzw) {
        geom_link.push_back(link);
        points.insert(points.end(), xyzw.begin(), xyzw.end());
        offsets.push_back((uint32_t)(points.size() / 4));
    }
    void allow(int32_t a, int32_t b) {
        allowed.push_back(a);
        allowed.push_back(b);
    }
    /* the description over the arrays as they stand; num_dofs < 0: the number of non-fixed joints (3 / 6) */
    const fks_robot_desc* desc(int32_t num_dofs = -1) {
        int32_t dofs = d.robot_type == FKS_ROBOT_SE2 ? 3 : 6;
        if (d.robot_type == FKS_ROBOT_LINKED) {
            dofs = 0;
            for (const fks_joint_desc& j : joints) dofs += j.type != FKS_JOINT_FIXED;
        }
        d.num_dofs = num_dofs < 0 ? dofs : num_dofs;
        d.num_joints = (int32_t)joints.size();
        d.num_geometries = (int32_t)geom_link.size();
        d.num_allowed_pairs = (int32_t)(allowed.size() / 2);
        ctrl.resize(64);
        if (points.empty()) points.reserve(4); /* a non-null array no test reads */
        d.joints = joints.data();
        d.geometry_link = geom_link.data();
        d.geometry_point_offset = offsets.data();
        d.points = points.data();
        d.allowed_pairs = allowed.data();
        d.controllers = ctrl.data();
        d.distance_weights = weights.empty() ? nullptr : weights.data();
        return &d;
    }
};

static bool flat_ok(Robot& r, Flat* f) {
    std::string why;
    const fks_status st = fks_robot::flatten(r.desc(), f, &why);
    if (st != FKS_OK) {
        std::fprintf(stderr, "flatten refused: %d \"%s\"\n", (int)st, why.c_str());
        ++g_failures;
    }
    return st == FKS_OK;
}

template <typename T>
static bool equal(const std::vector<T>& got, std::initializer_list<T> want) {
    return got == std::vector<T>(want);
}

/* dof_table numbers the dofs as flatten does, and carries the joints' types and limits */
static void check_dofs(Robot& r, const Flat& f) {
    std::vector<Dof> dofs;
    int W = -1;
    CHECK(fks_robot::dof_table(r.desc(), &dofs, &W) == FKS_OK);
    CHECK(W == f.R.W && W == f.R.D);
    CHECK(dofs.size() == f.dof_joint.size());
    int seen = 0;
    for (size_t j = 0; j < f.joints.size(); ++j) seen += f.joints[j].dof >= 0;
    CHECK(seen == (int)dofs.size());
    for (size_t k = 0; k < dofs.size() && k < f.dof_joint.size(); ++k) {
        CHECK(dofs[k].joint == f.dof_joint[k]);
        CHECK(f.joints[(size_t)dofs[k].joint].dof == (int32_t)k);
        const fks_joint_desc& jd = r.joints[(size_t)dofs[k].joint];
        CHECK(dofs[k].type == jd.type && dofs[k].lo == jd.limit_lower && dofs[k].hi == jd.limit_upper);
    }
}

/* The chain of the lever cases: link 0 -(joint 0, about z, at the origin)- link 1 -(joint 1, 0.5
 * along x)- link 2.  Geometry 0 on link 1: the point (0.5, 0, 0).  Geometry 1 on link 2: the points
 * (0.25, 0, 0) and (0, 0.1875, 0), whose box has centre and half extents (0.125, 0.09375, 0), each
 * of norm 0.15625 (3-4-5 in units of 0.03125). */
static Robot chain(int32_t type1 = FKS_JOINT_REVOLUTE, double az1 = 1.0, double lo1 = -1.0, double hi1 = 1.0, double w = 1.0) {
    Robot r(FKS_ROBOT_LINKED, 3);
    r.joint(0, 1, FKS_JOINT_REVOLUTE, 0, 0, 0, 0, 0, 1);
    r.joint(1, 2, type1, 0.5, 0, 0, 0, 0, az1, lo1, hi1);
    r.geometry(1, {0.5, 0, 0, 1});
    r.geometry(2, {0.25, 0, 0, 1, 0, 0.1875, 0, w});
    return r;
}

static void test_revolute_chain() {
    Robot r = chain();
    r.weights = {2.0, 0.5};
    Flat f;
    if (!flat_ok(r, &f)) return;
    CHECK(f.R.type == FKS_ROBOT_LINKED && f.R.L == 3 && f.R.J == 2 && f.R.G == 2 && f.R.D == 2 && f.R.P == 3 && f.R.W == 2);
    CHECK(std::memcmp(f.R.base, r.d.base_transform, sizeof(f.R.base)) == 0);
    CHECK(!f.R.joints && !f.R.points && !f.R.rounds && !f.R.dof_lever && !f.R.sampled && f.R.sampled_mask == 0);
    CHECK(f.joints.size() == 2);
    CHECK(f.joints[1].parent == 1 && f.joints[1].child == 2 && f.joints[1].type == FKS_JOINT_REVOLUTE && f.joints[1].dof == 1);
    CHECK(std::memcmp(f.joints[1].origin, r.joints[1].origin, sizeof(r.joints[1].origin)) == 0);
    CHECK(f.joints[1].axis[2] == 1.0 && f.joints[1].lo == -1.0 && f.joints[1].hi == 1.0);
    CHECK(equal(f.dof_joint, {0, 1}));
    CHECK(equal<uint64_t>(f.link_dof_mask, {0, 1, 3}));
    CHECK(equal<uint16_t>(f.point_geom, {0, 1, 1}));
    CHECK(equal<uint16_t>(f.point_link, {1, 2, 2}));
    CHECK(equal(f.geom_box, {0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.125, 0.09375, 0.0, 0.125, 0.09375, 0.0, 1.0}));
    CHECK(equal(f.geom_mass, {3.0, 2.0}));
    CHECK(equal(f.weights, {2.0, 0.5}));
    /* dof 0 moves both links: 0 + 0.5 on link 1; 0.5 + 0.25 and 0.5 + 0.1875 on link 2.  dof 1
     * moves link 2: 0 + 0.25, 0 + 0.1875 */
    CHECK(f.dof_lever.size() == 2 && f.dof_lever[0] == 0.75 * (1.0 + 1e-9) + 1e-12 && f.dof_lever[1] == 0.25 * (1.0 + 1e-9) + 1e-12);
    /* boxes: link 1 0 + 0.5 + 0; link 2 0.5 + 0.15625 + 0.15625 = 0.8125 from joint 0, 0.3125 from joint 1 */
    CHECK(f.dof_lever_box.size() == 2 && f.dof_lever_box[0] == 0.8125 * (1.0 + 1e-9) + 1e-12 &&
          f.dof_lever_box[1] == 0.3125 * (1.0 + 1e-9) + 1e-12);
    /* one round of three points on two links */
    CHECK(f.R.nrounds == 1 && f.rounds.size() == 1);
    CHECK(f.rounds[0].link == -1 && f.rounds[0].npts == 3 && f.rounds[0].radius == 0.5 * (1.0 + 1e-9) + 1e-12);
    check_dofs(r, f);
    /* no weights: 1 per dof */
    r.weights.clear();
    if (flat_ok(r, &f)) CHECK(equal(f.weights, {1.0, 1.0}));
}

static void test_prismatic_chain() {
    Robot r = chain(FKS_JOINT_PRISMATIC, 2.0, -0.25, 0.5);
    Flat f;
    if (!flat_ok(r, &f)) return;
    /* the prismatic dof: |axis| = 2, as it is */
    CHECK(f.dof_lever[1] == 2.0 && f.dof_lever_box[1] == 2.0);
    /* dof 0 reaches link 2 over the origin's 0.5 and the stroke max(0.25, 0.5) * 2 = 1: 1.5, then
     * 0.25 to the farthest point, 0.3125 to the box's corner bound */
    CHECK(f.dof_lever[0] == 1.75 * (1.0 + 1e-9) + 1e-12);
    CHECK(f.dof_lever_box[0] == 1.8125 * (1.0 + 1e-9) + 1e-12);
    CHECK(f.joints[1].type == FKS_JOINT_PRISMATIC && f.joints[1].lo == -0.25 && f.joints[1].hi == 0.5 && f.joints[1].axis[2] == 2.0);
    check_dofs(r, f);
}

static void test_non_unit_axis() {
    Robot r = chain(FKS_JOINT_REVOLUTE, 1.5);
    Flat f;
    if (!flat_ok(r, &f)) return;
    CHECK(f.dof_lever[1] == HUGE_VAL && f.dof_lever_box[1] == HUGE_VAL);
    CHECK(f.dof_lever[0] == 0.75 * (1.0 + 1e-9) + 1e-12 && f.dof_lever_box[0] == 0.8125 * (1.0 + 1e-9) + 1e-12);
    check_dofs(r, f);
}

static void test_w_not_one() {
    /* the chain with w = 0.5 on its last point, and a third link on the base with a point of its own */
    Robot r = chain(FKS_JOINT_REVOLUTE, 1.0, -1.0, 1.0, 0.5);
    r.d.num_links = 4;
    r.joint(0, 3, FKS_JOINT_REVOLUTE, 0, 0, 0, 1, 0, 0);
    r.geometry(3, {0, 0.25, 0, 1});
    Flat f;
    if (!flat_ok(r, &f)) return;
    CHECK(equal(f.dof_lever, {HUGE_VAL, HUGE_VAL, HUGE_VAL}));
    CHECK(f.geom_box[6] == 1.0 && f.geom_box[13] == 0.0 && f.geom_box[20] == 1.0);
    /* dofs 0 and 1 move the geometry without a box; dof 2 moves only link 3: 0 + 0.25 + 0 */
    CHECK(equal(f.dof_lever_box, {HUGE_VAL, HUGE_VAL, 0.25 * (1.0 + 1e-9) + 1e-12}));
    check_dofs(r, f);
    /* a round on one link: its link while every w is 1, -1 with one that is not; the radius either way */
    for (double w : {1.0, 0.5}) {
        Robot one(FKS_ROBOT_LINKED, 2);
        one.joint(0, 1, FKS_JOINT_CONTINUOUS, 0, 0, 0, 0, 0, 1);
        one.geometry(1, {0.5, 0, 0, 1, 0, 0, 2, w});
        if (!flat_ok(one, &f)) continue;
        CHECK(f.rounds[0].link == (w == 1.0 ? 1 : -1) && f.rounds[0].npts == 2);
        CHECK(f.rounds[0].radius == 2.0 * (1.0 + 1e-9) + 1e-12);
        CHECK(f.geom_box[6] == (w == 1.0 ? 1.0 : 0.0));
        CHECK(f.dof_lever[0] == (w == 1.0 ? 2.0 * (1.0 + 1e-9) + 1e-12 : HUGE_VAL));
    }
}

static void test_fixed_joint() {
    /* link 0 -(revolute)- link 1 -(fixed, 0.5 along x)- link 2 -(revolute, 0.25 along y)- link 3 */
    Robot r(FKS_ROBOT_LINKED, 4);
    r.joint(0, 1, FKS_JOINT_REVOLUTE, 0, 0, 0, 0, 0, 1);
    r.joint(1, 2, FKS_JOINT_FIXED, 0.5, 0, 0, 0, 0, 0);
    r.joint(2, 3, FKS_JOINT_CONTINUOUS, 0, 0.25, 0, 0, 1, 0, -0.5, 0.75);
    r.geometry(3, {0.25, 0, 0, 1});
    Flat f;
    if (!flat_ok(r, &f)) return;
    CHECK(f.R.J == 3 && f.R.D == 2 && f.R.W == 2);
    CHECK(equal(f.dof_joint, {0, 2}));
    CHECK(f.joints[0].dof == 0 && f.joints[1].dof == -1 && f.joints[2].dof == 1);
    CHECK(equal<uint64_t>(f.link_dof_mask, {0, 1, 1, 3}));
    /* dof 0: 0.25 + 0.5 over the two joints below it, then 0.25; dof 1: 0.25 */
    CHECK(equal(f.dof_lever, {1.0 * (1.0 + 1e-9) + 1e-12, 0.25 * (1.0 + 1e-9) + 1e-12}));
    CHECK(equal(f.dof_lever_box, {1.0 * (1.0 + 1e-9) + 1e-12, 0.25 * (1.0 + 1e-9) + 1e-12}));
    CHECK(f.rounds[0].link == 3 && f.rounds[0].npts == 1 && f.rounds[0].radius == 0.25 * (1.0 + 1e-9) + 1e-12);
    check_dofs(r, f);
    std::vector<Dof> dofs;
    int W = 0;
    CHECK(fks_robot::dof_table(r.desc(), &dofs, &W) == FKS_OK && W == 2 && dofs.size() == 2);
    CHECK(dofs[1].joint == 2 && dofs[1].type == FKS_JOINT_CONTINUOUS && dofs[1].lo == -0.5 && dofs[1].hi == 0.75);
}

static void test_branched_tree() {
    /* link 1 on the base carries links 2 and 3; link 4 slides on the base */
    Robot r(FKS_ROBOT_LINKED, 5);
    r.joint(0, 1, FKS_JOINT_REVOLUTE, 0, 0, 0, 0, 0, 1);
    r.joint(1, 2, FKS_JOINT_REVOLUTE, 0, 0, 0, 0, 1, 0);
    r.joint(1, 3, FKS_JOINT_REVOLUTE, 0, 0, 0.25, 1, 0, 0);
    r.joint(0, 4, FKS_JOINT_PRISMATIC, 0, 0, 0, 1, 0, 0);
    r.geometry(2, {0.5, 0, 0, 1});
    r.geometry(3, {0.25, 0, 0, 1});
    r.geometry(4, {2, 0, 0, 1});
    Flat f;
    if (!flat_ok(r, &f)) return;
    CHECK(equal<uint64_t>(f.link_dof_mask, {0x0, 0x1, 0x3, 0x5, 0x8}));
    CHECK(equal(f.dof_joint, {0, 1, 2, 3}));
    /* dof 0: link 2 0 + 0.5, link 3 0.25 + 0.25; dof 1: link 2 alone; dof 2: link 3 alone; dof 3: |axis| */
    CHECK(equal(f.dof_lever, {0.5 * (1.0 + 1e-9) + 1e-12, 0.5 * (1.0 + 1e-9) + 1e-12, 0.25 * (1.0 + 1e-9) + 1e-12, 1.0}));
    CHECK(f.dof_lever_box == f.dof_lever); /* one point per geometry: the box is the point */
    check_dofs(r, f);
}

static void test_rounds() {
    /* the chain's links with `first` points on link 1, one of them at (0, 1.5, 2) (norm 2.5), then
     * (0.25, 0, 0) and, if `second` is 2, (0, 0.1875, 0) on link 2 */
    for (int first : {64, 63}) {
        Robot r(FKS_ROBOT_LINKED, 3);
        r.joint(0, 1, FKS_JOINT_REVOLUTE, 0, 0, 0, 0, 0, 1);
        r.joint(1, 2, FKS_JOINT_REVOLUTE, 0.5, 0, 0, 0, 0, 1);
        r.geometry(1, {});
        for (int i = 0; i < first; ++i) {
            const double p[4] = {i == 10 ? 0.0 : 0.5, i == 10 ? 1.5 : 0.0, i == 10 ? 2.0 : 0.0, 1.0};
            r.points.insert(r.points.end(), p, p + 4);
        }
        r.offsets.back() = (uint32_t)first;
        if (first == 64)
            r.geometry(2, {0.25, 0, 0, 1});
        else
            r.geometry(2, {0.25, 0, 0, 1, 0, 0.1875, 0, 1});
        Flat f;
        if (!flat_ok(r, &f)) continue;
        CHECK(f.R.P == 65 && f.R.nrounds == 2 && f.rounds.size() == 2);
        CHECK(f.rounds[0].npts == 64 && f.rounds[0].radius == 2.5 * (1.0 + 1e-9) + 1e-12);
        CHECK(f.rounds[0].link == (first == 64 ? 1 : -1)); /* 63 + 1: mixed */
        CHECK(f.rounds[1].npts == 1 && f.rounds[1].link == 2);
        CHECK(f.rounds[1].radius == (first == 64 ? 0.25 : 0.1875) * (1.0 + 1e-9) + 1e-12);
        CHECK(f.point_link[62] == 1 && f.point_link[63] == (first == 64 ? 1 : 2) && f.point_link[64] == 2);
        CHECK(f.point_geom[62] == 0 && f.point_geom[64] == 1);
        check_dofs(r, f);
    }
}

static void test_empty_geometry() {
    Robot r(FKS_ROBOT_LINKED, 3);
    r.joint(0, 1, FKS_JOINT_REVOLUTE, 0, 0, 0, 0, 0, 1);
    r.joint(1, 2, FKS_JOINT_REVOLUTE, 0.5, 0, 0, 0, 0, 1);
    r.geometry(1, {0.5, 0, 0, 1});
    r.geometry(1, {});
    r.geometry(2, {0.25, 0, 0, 1, -0.25, 0, 0, 1});
    Flat f;
    if (!flat_ok(r, &f)) return;
    CHECK(equal(f.geom_box, {0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 1.0}));
    /* points of the geometry and of every later one: 1 + 0 + 2, 0 + 2, 2 */
    CHECK(equal(f.geom_mass, {3.0, 2.0, 2.0}));
    CHECK(equal<uint16_t>(f.point_geom, {0, 2, 2}));
    /* the empty box adds 0 + 0 + 0 to dof 0's box lever: link 1 0.5, link 2 0.5 + 0 + 0.25 */
    CHECK(f.dof_lever_box[0] == 0.75 * (1.0 + 1e-9) + 1e-12);
}

static void test_allowed_pairs() {
    auto robot = [](int G) {
        Robot r(FKS_ROBOT_LINKED, 2);
        r.joint(0, 1, FKS_JOINT_REVOLUTE, 0, 0, 0, 0, 0, 1);
        for (int g = 0; g < G; ++g) r.geometry(g % 2, {0.25, 0, 0, 1});
        return r;
    };
    Flat f;
    Robot four = robot(4);
    four.allow(0, 1);
    four.allow(1, 0); /* both orders */
    four.allow(2, 3);
    four.allow(2, 3); /* twice */
    if (flat_ok(four, &f)) {
        CHECK(equal<uint64_t>(f.allowed_mask, {0x3, 0x3, 0xc, 0xc}));
        CHECK(equal(f.pairs, {0, 2, 0, 3, 1, 2, 1, 3}));
        CHECK(f.R.npairs == 4 && f.R.self_possible == 1);
    }
    Robot one = robot(1);
    if (flat_ok(one, &f)) {
        CHECK(equal<uint64_t>(f.allowed_mask, {0x1}) && f.pairs.empty() && f.R.npairs == 0 && f.R.self_possible == 0);
    }
    Robot two = robot(2);
    if (flat_ok(two, &f)) {
        CHECK(equal<uint64_t>(f.allowed_mask, {0x1, 0x2}) && equal(f.pairs, {0, 1}) && f.R.npairs == 1 && f.R.self_possible == 1);
    }
    two.allow(1, 0);
    if (flat_ok(two, &f)) {
        CHECK(equal<uint64_t>(f.allowed_mask, {0x3, 0x3}) && f.pairs.empty() && f.R.npairs == 0 && f.R.self_possible == 0);
    }
}

static Robot body(int32_t type) {
    Robot r(type);
    r.geometry(0, {0.5, 0, 0, 1, 0, 1.5, 2, 1}); /* norms 0.5 and 2.5 */
    return r;
}

static void test_free_bodies() {
    for (int32_t type : {FKS_ROBOT_SE2, FKS_ROBOT_SE3}) {
        const bool se2 = type == FKS_ROBOT_SE2;
        Robot r = body(type);
        r.weights = {0.5, 4.0};
        Flat f;
        if (!flat_ok(r, &f)) continue;
        CHECK(f.R.type == type && f.R.L == 1 && f.R.J == 0 && f.R.G == 1 && f.R.P == 2);
        CHECK(f.R.D == (se2 ? 3 : 6) && f.R.W == (se2 ? 3 : 12));
        CHECK(f.joints.empty() && f.dof_joint.empty() && equal<uint64_t>(f.link_dof_mask, {0}));
        if (se2)
            CHECK(equal(f.dof_lever, {1.0 + 1e-9, 1.0 + 1e-9, 2.5 * (1.0 + 1e-9) + 1e-12}));
        else
            CHECK(equal(f.dof_lever, {1.0 + 1e-9, 1.0 + 1e-9, 1.0 + 1e-9, 2.5 * (1.0 + 1e-9) + 1e-12, 2.5 * (1.0 + 1e-9) + 1e-12,
                                      2.5 * (1.0 + 1e-9) + 1e-12}));
        CHECK(f.dof_lever_box == std::vector<double>(se2 ? 3 : 6, HUGE_VAL));
        CHECK(equal(f.weights, {0.5, 4.0}));
        CHECK(f.rounds.size() == 1 && f.rounds[0].link == 0 && f.rounds[0].npts == 2 && f.rounds[0].radius == 2.5 * (1.0 + 1e-9) + 1e-12);
        CHECK(f.R.npairs == 0 && f.R.self_possible == 0);
        std::vector<Dof> dofs(3);
        int W = 0;
        CHECK(fks_robot::dof_table(r.desc(), &dofs, &W) == FKS_OK && W == (se2 ? 3 : 12) && dofs.empty());
        r.weights.clear();
        if (flat_ok(r, &f)) CHECK(equal(f.weights, {1.0, 1.0}));
        /* a w != 1: no lever */
        r.points[7] = 0.5;
        if (flat_ok(r, &f)) {
            CHECK(f.dof_lever == std::vector<double>(se2 ? 3 : 6, HUGE_VAL));
            CHECK(f.rounds[0].link == -1);
        }
    }
}

static void refused(const fks_robot_desc* d, const char* text) {
    Flat f;
    std::string why;
    const fks_status st = fks_robot::flatten(d, &f, &why);
    if (st != FKS_ERR_INVALID_ARGUMENT || why != text) {
        std::fprintf(stderr, "refusal: got %d \"%s\", want %d \"%s\"\n", (int)st, why.c_str(), (int)FKS_ERR_INVALID_ARGUMENT, text);
        ++g_failures;
    }
}

static void test_refusals() {
    const char* missing = "robot geometries/controllers missing or more than 64 geometries";
    {
        Robot r(FKS_ROBOT_LINKED, 2);
        r.joint(0, 1, FKS_JOINT_REVOLUTE, 0, 0, 0, 0, 0, 1);
        refused(r.desc(), missing); /* no geometry */
        for (int g = 0; g < 65; ++g) r.geometry(1, {0.25, 0, 0, 1});
        refused(r.desc(), missing);
    }
    for (int which = 0; which < 4; ++which) {
        Robot r = chain();
        fks_robot_desc d = *r.desc();
        if (which == 0) d.geometry_link = nullptr;
        if (which == 1) d.geometry_point_offset = nullptr;
        if (which == 2) d.points = nullptr;
        if (which == 3) d.controllers = nullptr;
        refused(&d, missing);
    }
    const char* count = "robot needs 1..65535 points with offsets starting at 0";
    {
        Robot r = chain();
        r.offsets[0] = 1;
        refused(r.desc(), count);
        r.offsets = {0, 0, 0};
        refused(r.desc(), count);
        r.offsets = {0, 1, 65536}; /* refused before a point is read */
        refused(r.desc(), count);
        r.offsets = {0, 3, 2};
        refused(r.desc(), "geometry offsets must be non-decreasing");
    }
    for (double bad : {kNaN, kInf, -kInf}) {
        Robot r = chain();
        r.points[9] = bad;
        refused(r.desc(), "non-finite robot point");
        r = chain();
        r.points[11] = bad; /* a w */
        refused(r.desc(), "non-finite robot point");
    }
    const char* sizes = "linked robot needs 1..64 links and 0..64 joints";
    {
        Robot r = chain();
        r.d.num_links = 0;
        refused(r.desc(), sizes);
        r.d.num_links = 65;
        refused(r.desc(), sizes);
        r.d.num_links = 3;
        fks_robot_desc d = *r.desc();
        d.num_joints = -1;
        refused(&d, sizes);
        d.num_joints = 65;
        refused(&d, sizes);
        d.num_joints = 2;
        d.joints = nullptr;
        refused(&d, sizes);
    }
    const char* range = "joint link index out of range";
    for (int which = 0; which < 4; ++which) {
        Robot r = chain();
        if (which == 0) r.joints[1].parent_link = -1;
        if (which == 1) r.joints[1].parent_link = 3;
        if (which == 2) r.joints[1].child_link = 0;
        if (which == 3) r.joints[1].child_link = 3;
        refused(r.desc(), range);
    }
    const char* order = "joints must be in topological order, one parent per link";
    {
        Robot r = chain();
        std::swap(r.joints[0], r.joints[1]); /* link 1's joint after the joint that hangs from it */
        refused(r.desc(), order);
        r = chain();
        r.joints[1].child_link = 1; /* a second parent */
        refused(r.desc(), order);
    }
    {
        Robot r = chain();
        r.joints[1].type = 3;
        refused(r.desc(), "unknown joint type");
        r = chain();
        r.d.num_links = 4;
        refused(r.desc(), "every link must be reached by a joint");
    }
    const char* dofs = "num_dofs must equal the number of non-fixed joints (1..64)";
    {
        Robot r = chain();
        refused(r.desc(1), dofs);
        refused(r.desc(3), dofs);
        r.joints[0].type = FKS_JOINT_FIXED;
        r.joints[1].type = FKS_JOINT_FIXED;
        refused(r.desc(0), dofs);
        Robot lone(FKS_ROBOT_LINKED, 1); /* a base and nothing else */
        lone.geometry(0, {0.25, 0, 0, 1});
        refused(lone.desc(0), dofs);
    }
    for (int32_t link : {-1, 3}) {
        Robot r = chain();
        r.geom_link[1] = link;
        refused(r.desc(), "geometry link index out of range");
    }
    const char* bodies = "SE(2)/SE(3) robots have one geometry on link 0 and 3/6 dofs";
    for (int32_t type : {FKS_ROBOT_SE2, FKS_ROBOT_SE3}) {
        Robot r = body(type);
        refused(r.desc(type == FKS_ROBOT_SE2 ? 6 : 3), bodies);
        refused(r.desc(type == FKS_ROBOT_SE2 ? 2 : 12), bodies);
        r.geom_link[0] = 1;
        refused(r.desc(), bodies);
        r.geom_link[0] = 0;
        r.geometry(0, {0.25, 0, 0, 1});
        refused(r.desc(), bodies);
    }
    {
        Robot r = body(7);
        refused(r.desc(), "unknown robot type");
        r = body(-1);
        refused(r.desc(), "unknown robot type");
    }
    for (int which = 0; which < 4; ++which) {
        Robot r = chain();
        const int32_t pair[4][2] = {{-1, 0}, {0, -1}, {2, 0}, {1, 2}};
        r.allow(0, 1);
        r.allow(pair[which][0], pair[which][1]);
        refused(r.desc(), "allowed pair out of range");
    }
    /* sampled actuators: dof 0 keeps its truncated-normal actuator, dof 1 has two bins of three samples */
    {
        Robot r = chain();
        double bounds[4] = {-1.0, 0.0, 0.0, 1.0};
        double samples[6] = {0.0, 0.125, -0.125, 0.25, 0.0, -0.25};
        fks_sampled_actuator sa[2];
        std::memset(sa, 0, sizeof(sa));
        sa[1].num_bins = 2;
        sa[1].bin_elements = 3;
        sa[1].bin_bounds = bounds;
        sa[1].bin_samples = samples;
        fks_robot_desc d = *r.desc();
        d.sampled_actuators = sa;
        Flat f;
        std::string why;
        CHECK(fks_robot::flatten(&d, &f, &why) == FKS_OK);
        CHECK(f.R.sampled_mask == 0 && !f.R.sampled); /* the tables are the caller's: fks_set_robot uploads them */
        bounds[1] = kInf; /* an open bin is fine */
        CHECK(fks_robot::flatten(&d, &f, &why) == FKS_OK);
        const char* tables = "sampled actuator needs bounds and >= 1 sample per bin";
        sa[1].bin_elements = 0;
        refused(&d, tables);
        sa[1].bin_elements = 3;
        sa[1].bin_bounds = nullptr;
        refused(&d, tables);
        sa[1].bin_bounds = bounds;
        sa[1].bin_samples = nullptr;
        refused(&d, tables);
        sa[1].bin_samples = samples;
        bounds[3] = kNaN;
        refused(&d, "NaN sampled-actuator bin bound");
        bounds[3] = 1.0;
        samples[5] = kNaN;
        refused(&d, "non-finite sampled-actuator sample");
        samples[5] = kInf;
        refused(&d, "non-finite sampled-actuator sample");
    }
}

static void test_dof_table_refusals() {
    std::vector<Dof> dofs;
    int W = 0;
    CHECK(fks_robot::dof_table(nullptr, &dofs, &W) == FKS_ERR_INVALID_ARGUMENT);
    Robot r = chain();
    fks_robot_desc d = *r.desc();
    d.num_joints = -1;
    CHECK(fks_robot::dof_table(&d, &dofs, &W) == FKS_ERR_INVALID_ARGUMENT);
    d.num_joints = 2;
    d.joints = nullptr;
    CHECK(fks_robot::dof_table(&d, &dofs, &W) == FKS_ERR_INVALID_ARGUMENT);
    CHECK(fks_robot::dof_table(r.desc(1), &dofs, &W) == FKS_ERR_INVALID_ARGUMENT);
    CHECK(fks_robot::dof_table(r.desc(3), &dofs, &W) == FKS_ERR_INVALID_ARGUMENT);
    r.joints[0].type = FKS_JOINT_FIXED;
    r.joints[1].type = FKS_JOINT_FIXED;
    CHECK(fks_robot::dof_table(r.desc(0), &dofs, &W) == FKS_ERR_INVALID_ARGUMENT);
    for (int32_t type : {FKS_ROBOT_SE2, FKS_ROBOT_SE3}) {
        Robot b = body(type);
        CHECK(fks_robot::dof_table(b.desc(type == FKS_ROBOT_SE2 ? 6 : 3), &dofs, &W) == FKS_ERR_INVALID_ARGUMENT);
        CHECK(fks_robot::dof_table(b.desc(12), &dofs, &W) == FKS_ERR_INVALID_ARGUMENT);
    }
    Robot unknown = body(7);
    CHECK(fks_robot::dof_table(unknown.desc(3), &dofs, &W) == FKS_ERR_INVALID_ARGUMENT);
    /* what it does not need: geometries, controllers, weights */
    Robot bare(FKS_ROBOT_LINKED, 2);
    bare.joint(0, 1, FKS_JOINT_PRISMATIC, 0, 0, 0, 1, 0, 0, -2.0, 0.5);
    std::memset(&d, 0, sizeof(d));
    d.robot_type = FKS_ROBOT_LINKED;
    d.num_joints = 1;
    d.num_dofs = 1;
    d.joints = bare.joints.data();
    CHECK(fks_robot::dof_table(&d, &dofs, &W) == FKS_OK && W == 1 && dofs.size() == 1);
    CHECK(dofs[0].joint == 0 && dofs[0].type == FKS_JOINT_PRISMATIC && dofs[0].lo == -2.0 && dofs[0].hi == 0.5);
}

/* a field of nx x ny x nz cells (z fastest) in a block of exactly that size */
static std::vector<float> field(int nx, int ny, int nz, float (*value)(int, int, int)) {
    std::vector<float> v;
    for (int x = 0; x < nx; ++x)
        for (int y = 0; y < ny; ++y)
            for (int z = 0; z < nz; ++z) v.push_back(value(x, y, z));
    return v;
}

static void test_analyze_sdf() {
    const double res = 0.5;
    double lp = -1.0, cm = -1.0;
    /* the distance to the plane x = 0, in cells: 0, res, 2 res.  Positive neighbours differ by res;
     * the positive cells beside a non-positive one hold res */
    std::vector<float> v = field(3, 3, 3, [](int x, int, int) { return 0.5f * (float)x; });
    CHECK(fks_robot::analyze_sdf(v.data(), 3, 3, 3, res, &lp, &cm) && lp == 1.0 && cm == 1.0);
    /* (2, 1, 1) raised from 2 res to 4 res: 3 res above (1, 1, 1) */
    v[(2 * 3 + 1) * 3 + 1] = 2.0f;
    CHECK(fks_robot::analyze_sdf(v.data(), 3, 3, 3, res, &lp, &cm) && lp == 3.0 && cm == 1.0);
    /* a positive cell of 3 res beside a non-positive one */
    v = field(3, 3, 3, [](int x, int, int) { return 0.5f * (float)x; });
    v[(1 * 3 + 1) * 3 + 1] = 1.5f;
    CHECK(fks_robot::analyze_sdf(v.data(), 3, 3, 3, res, &lp, &cm) && lp == 2.0 && cm == 3.0);
    /* one NaN, one infinity */
    for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
        v = field(3, 3, 3, [](int x, int, int) { return 0.5f * (float)x; });
        v[26] = bad;
        CHECK(!fks_robot::analyze_sdf(v.data(), 3, 3, 3, res, &lp, &cm));
    }
    /* no pair of positive neighbours: nothing positive, and positive cells that never touch */
    v = field(3, 3, 3, [](int, int, int) { return -0.5f; });
    CHECK(!fks_robot::analyze_sdf(v.data(), 3, 3, 3, res, &lp, &cm) && lp == 0.0 && cm == 0.0);
    v = field(3, 3, 3, [](int x, int y, int z) { return (x == 1 && y == 1 && z == 1) ? 0.5f : 0.0f; });
    CHECK(!fks_robot::analyze_sdf(v.data(), 3, 3, 3, res, &lp, &cm) && lp == 0.0 && cm == 1.0);
    /* an extent of 1 along each axis in turn: no neighbour is read past the block */
    v = field(1, 3, 3, [](int, int y, int) { return 0.5f * (float)y; });
    CHECK(fks_robot::analyze_sdf(v.data(), 1, 3, 3, res, &lp, &cm) && lp == 1.0 && cm == 1.0);
    v = field(3, 1, 3, [](int, int, int z) { return 0.5f * (float)z; });
    CHECK(fks_robot::analyze_sdf(v.data(), 3, 1, 3, res, &lp, &cm) && lp == 1.0 && cm == 1.0);
    v = field(3, 3, 1, [](int x, int, int) { return 0.5f * (float)x; });
    CHECK(fks_robot::analyze_sdf(v.data(), 3, 3, 1, res, &lp, &cm) && lp == 1.0 && cm == 1.0);
    v = field(1, 1, 3, [](int, int, int z) { return 0.5f * (float)z; });
    CHECK(fks_robot::analyze_sdf(v.data(), 1, 1, 3, res, &lp, &cm) && lp == 1.0 && cm == 1.0);
}

int main() {
    test_revolute_chain();
    test_prismatic_chain();
    test_non_unit_axis();
    test_w_not_one();
    test_fixed_joint();
    test_branched_tree();
    test_rounds();
    test_empty_geometry();
    test_allowed_pairs();
    test_free_bodies();
    test_refusals();
    test_dof_table_refusals();
    test_analyze_sdf();
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("robot flatten test ok\n");
    return 0;
}
