/*
 * select_plan_test.cpp — the host-side plan of a state selection (fks_batch::plan_select) and the
 * host twin fks_select_states without a GPU: every refusal's status and text, the invariants of
 * the decomposition over a sweep of queries, states and compute-unit counts, and the twin on a
 * one-dof prismatic robot of weight 1 (every distance exact) with exactly-sized heap buffers, so
 * the sanitizer watches their ends: the guard case sits at the pool's last row.  Links only the
 * HIP-free units fks_batch.cpp, fks_state_select.cpp, fks_policy_select.cpp and fks_robot.cpp.
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

static fks_state_table table_of(const double* keys, uint64_t S) {
    fks_state_table t;
    std::memset(&t, 0, sizeof(t));
    t.keys = keys;
    t.num_states = S;
    return t;
}

static bool refused(const fks_state_table* t, const double* queries, uint64_t J, uint32_t P, const fks_state_selection* out,
                    const char* text) {
    SelectPlan p;
    std::string why;
    const fks_status st = plan_select(&p, 3, 256, t, queries, J, P, out, &why);
    if (st != FKS_ERR_INVALID_ARGUMENT || why.find(text) == std::string::npos) {
        std::fprintf(stderr, "expected \"%s\", got status %d \"%s\"\n", text, (int)st, why.c_str());
        return false;
    }
    return true;
}

static void test_refusals() {
    double q[4]; /* never dereferenced */
    uint32_t u[4];
    fks_state_selection choice_only;
    std::memset(&choice_only, 0, sizeof(choice_only));
    choice_only.choice = u;
    fks_state_selection with_starts = choice_only, with_source = choice_only, nothing;
    with_starts.starts = q;
    with_source.source = u;
    std::memset(&nothing, 0, sizeof(nothing));
    fks_state_table plain = table_of(q, 5);
    fks_state_table full = plain;
    full.count = u;
    full.begin = u;
    full.members = q;
    full.num_member_rows = 9;
    SelectPlan p;
    std::string why;
    CHECK(plan_select(&p, 3, 256, &plain, q, 4, 0, &choice_only, &why) == FKS_OK && p.launch && !p.draw);
    CHECK(plan_select(&p, 3, 256, &full, q, 4, 2, &with_starts, &why) == FKS_OK && p.draw && p.particles == 2);
    CHECK(plan_select(&p, 3, 256, &full, q, 4, 2, &with_source, &why) == FKS_OK && p.draw);
    /* P is not read when nothing is drawn */
    CHECK(plan_select(&p, 3, 256, &full, q, 4, 0, &choice_only, &why) == FKS_OK && !p.draw);
    /* no query: nothing to launch, and neither queries nor choice is asked for */
    CHECK(plan_select(&p, 3, 256, &plain, nullptr, 0, 0, &nothing, &why) == FKS_OK && !p.launch);
    /* the bounds themselves pass */
    fks_state_table most = table_of(q, FKS_MAX_STATES);
    CHECK(plan_select(&p, 3, 256, &most, q, 1, 0, &choice_only, &why) == FKS_OK);
    CHECK(plan_select(&p, 3, 256, &full, q, 1ull << 20, 2048, &with_starts, &why) == FKS_OK);
    CHECK(plan_select(&p, 3, 256, &full, q, 1ull << 15, 65536, &with_starts, &why) == FKS_OK);

    CHECK(refused(nullptr, q, 4, 0, &choice_only, "null state table"));
    CHECK(refused(&plain, q, 4, 0, nullptr, "null selection"));
    fks_state_table no_keys = table_of(nullptr, 5);
    CHECK(refused(&no_keys, q, 4, 0, &choice_only, "null keys"));
    fks_state_table empty = table_of(q, 0);
    CHECK(refused(&empty, q, 4, 0, &choice_only, "at least one state"));
    fks_state_table over = table_of(q, FKS_MAX_STATES + 1);
    CHECK(refused(&over, q, 4, 0, &choice_only, "2^30"));
    CHECK(refused(&plain, q, 4, 0, &nothing, "null choice"));
    CHECK(refused(&plain, nullptr, 4, 0, &choice_only, "null queries"));
    CHECK(refused(&full, q, 4, 0, &with_starts, "num_particles == 0"));
    CHECK(refused(&full, q, 4, 0, &with_source, "num_particles == 0"));
    for (int drop = 0; drop < 3; ++drop) {
        fks_state_table t = full;
        if (drop == 0) t.count = nullptr, t.begin = nullptr; /* (begin without count has its own refusal) */
        if (drop == 1) t.begin = nullptr;
        if (drop == 2) t.members = nullptr;
        CHECK(refused(&t, q, 4, 2, &with_starts, "without count, begin and members"));
        CHECK(refused(&t, q, 4, 2, &with_source, "without count, begin and members"));
    }
    fks_state_table begin_only = plain;
    begin_only.begin = u;
    CHECK(refused(&begin_only, q, 4, 0, &choice_only, "begin is given without count"));
    CHECK(refused(&plain, q, (1ull << 20) + 1, 0, &choice_only, "2^20"));
    CHECK(refused(&full, q, 4, 65537, &with_starts, "65536"));
    CHECK(refused(&full, q, (1ull << 20), 2049, &with_starts, "2^31"));
}

/* chunks x chunk size covers S, every chunk holds a state, the workspace is one partial per (query, chunk) */
static void test_invariants() {
    double q[1];
    uint32_t u[1];
    fks_state_selection out;
    std::memset(&out, 0, sizeof(out));
    out.choice = u;
    const uint64_t Js[] = {1, 7, 8, 9, 64, 70, 1000, 8192, 8193, 1ull << 20};
    const uint64_t Ss[] = {1, 63, 255, 256, 257, 600, 1000, 50000, 70000, 1000003, FKS_MAX_STATES};
    const int32_t cus[] = {0, 1, 8, 104, 256, 304};
    for (uint64_t J : Js)
        for (uint64_t S : Ss)
            for (int32_t cu : cus) {
                fks_state_table t = table_of(q, S);
                SelectPlan p;
                std::string why;
                CHECK(plan_select(&p, 3, cu, &t, q, J, 0, &out, &why) == FKS_OK);
                CHECK(p.tile == (J < 8 ? J : 8) && p.tiles == (J + 7) / 8);
                CHECK(p.chunk_states > 0 && p.chunk_states % 256 == 0);
                CHECK(p.chunks >= 1 && p.chunks * p.chunk_states >= S);
                CHECK((p.chunks - 1) * p.chunk_states < S); /* the last chunk holds a state */
                CHECK(p.groups == p.tiles * p.chunks && p.groups < (1ull << 31));
                CHECK(p.work_partials == J * p.chunks);
                const uint64_t want = 4 * (uint64_t)(cu < 1 ? 1 : cu);
                CHECK(p.chunks <= (want + p.tiles - 1) / p.tiles); /* no more chunks than the rule asks for */
                if (S <= 256 || p.tiles >= want) CHECK(p.chunks == 1);
            }
    /* the cases the GPU test relies on */
    fks_state_table t600 = table_of(q, 600), t70k = table_of(q, 70000);
    SelectPlan p;
    std::string why;
    CHECK(plan_select(&p, 3, 256, &t600, q, 1, 0, &out, &why) == FKS_OK && p.chunks == 3 && p.chunk_states == 256);
    CHECK(plan_select(&p, 3, 256, &t70k, q, 70, 0, &out, &why) == FKS_OK && p.chunks > 1);
    uint64_t info[4];
    CHECK(fks_select_states_plan(70, 70000, 256, info) == FKS_OK && info[0] == 8 && info[1] == p.chunk_states && info[2] == p.chunks &&
          info[3] == p.groups);
    CHECK(fks_select_states_plan(70, 0, 256, info) == FKS_ERR_INVALID_ARGUMENT);
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

typedef std::vector<uint32_t> L;
typedef std::vector<double> D;

/* every output of one call on exactly-sized heap buffers */
struct Outputs {
    L choice, source;
    D distance, starts;
    fks_state_selection s;
    Outputs(size_t J, size_t P) : choice(J, 99u), source(J * P, 99u), distance(J, -1.0), starts(J * P, -1.0) {
        s.choice = choice.data();
        s.distance = distance.data();
        s.starts = P ? starts.data() : nullptr;
        s.source = P ? source.data() : nullptr;
    }
};

static void test_twin() {
    fks_joint_desc joint;
    fks_dof_controller ctrl;
    const double one = 1.0;
    const fks_robot_desc r = slider(&joint, &ctrl, &one);
    {
        /* four states over a pool of six rows; the last state ends exactly at the pool's end */
        const D keys = {0.0, 10.0, 20.0, 30.0}, weights = {1.0, 1.0, 0.5, 1.0};
        const L count = {2, 0, 1, 3}, begin = {0, 2, 2, 3};
        const D members = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0};
        fks_state_table t = table_of(keys.data(), 4);
        t.weights = weights.data();
        t.count = count.data();
        t.begin = begin.data();
        t.members = members.data();
        t.num_member_rows = 6;
        const D queries = {1.0, 10.0, 29.0, 14.0};
        Outputs o(4, 3);
        CHECK(fks_select_states(&r, &t, queries.data(), 4, 3, 5, &o.s) == FKS_OK);
        /* 10.0 is state 1's key, but state 1 is empty: state 2 at 0.5 x 10 = 5 beats state 0 at 10 */
        CHECK((o.choice == L{0, 2, 3, 2}) && (o.distance == D{1.0, 5.0, 1.0, 3.0}));
        for (size_t k = 0; k < 3; ++k) {
            CHECK(o.source[k] < 2 && o.starts[k] == members[o.source[k]]); /* c = 2 != P: drawn from rows 0, 1 */
            CHECK(o.source[3 + k] == 2 && o.starts[3 + k] == 3.0);        /* c = 1: the one member */
            CHECK(o.source[6 + k] == 3 + k && o.starts[6 + k] == 4.0 + (double)k); /* c == P: in order, to the last row */
            CHECK(o.source[9 + k] == 2 && o.starts[9 + k] == 3.0);
        }
        /* one row fewer in the pool: state 3 trips the guard, and nothing of row 5 is read (the buffer ends there) */
        const D shorter(members.begin(), members.begin() + 5);
        t.members = shorter.data();
        t.num_member_rows = 5;
        Outputs g(4, 3);
        CHECK(fks_select_states(&r, &t, queries.data(), 4, 3, 5, &g.s) == FKS_OK);
        CHECK((g.choice == L{0, 2, 3, 2}) && (g.distance == D{1.0, 5.0, 1.0, 3.0}));
        for (size_t k = 0; k < 3; ++k) {
            CHECK(g.source[6 + k] == FKS_STATE_NONE && g.starts[6 + k] == 0.0 && !std::signbit(g.starts[6 + k]));
            CHECK(g.source[k] == o.source[k] && g.source[3 + k] == 2 && g.source[9 + k] == 2); /* its neighbours are served */
        }
        /* selection only: no count, no draw; the empty state is then a state */
        fks_state_table bare = table_of(keys.data(), 4);
        Outputs b(4, 0);
        CHECK(fks_select_states(&r, &bare, queries.data(), 4, 0, 0, &b.s) == FKS_OK);
        CHECK((b.choice == L{0, 1, 3, 1}) && (b.distance == D{1.0, 0.0, 1.0, 4.0}));
        /* source without starts, and without distance */
        Outputs so(4, 3);
        so.s.starts = nullptr;
        so.s.distance = nullptr;
        CHECK(fks_select_states(&r, &t, queries.data(), 4, 3, 5, &so.s) == FKS_OK);
        CHECK(so.source == g.source && so.distance[0] == -1.0 && so.starts[0] == -1.0);
        /* no winner */
        const L none = {0, 0, 0, 0};
        t.count = none.data();
        Outputs n(4, 3);
        CHECK(fks_select_states(&r, &t, queries.data(), 4, 3, 5, &n.s) == FKS_OK);
        for (size_t j = 0; j < 4; ++j) CHECK(n.choice[j] == FKS_STATE_NONE && n.distance[j] == kInf);
        for (size_t k = 0; k < 12; ++k) CHECK(n.source[k] == FKS_STATE_NONE && n.starts[k] == 0.0);
    }
    {
        /* refusals of the entry itself */
        const D keys = {0.0}, queries = {1.0};
        fks_state_table t = table_of(keys.data(), 1);
        Outputs o(1, 0);
        CHECK(fks_select_states(nullptr, &t, queries.data(), 1, 0, 0, &o.s) == FKS_ERR_INVALID_ARGUMENT);
        fks_robot_desc bad = r;
        bad.num_dofs = 2;
        CHECK(fks_select_states(&bad, &t, queries.data(), 1, 0, 0, &o.s) == FKS_ERR_INVALID_ARGUMENT);
        CHECK(fks_select_states(&r, nullptr, queries.data(), 1, 0, 0, &o.s) == FKS_ERR_INVALID_ARGUMENT);
        CHECK(fks_select_states(&r, &t, queries.data(), 1, 0, 0, nullptr) == FKS_ERR_INVALID_ARGUMENT);
        CHECK(fks_select_states(&r, &t, nullptr, 1, 0, 0, &o.s) == FKS_ERR_INVALID_ARGUMENT);
        CHECK(o.choice[0] == 99u);
        CHECK(fks_select_states(&r, &t, nullptr, 0, 0, 0, &o.s) == FKS_OK && o.choice[0] == 99u);
    }
    {
        /* Philox4x32-10: the Random123 known answers */
        const uint32_t c0[4] = {0, 0, 0, 0}, k0[2] = {0, 0};
        const uint32_t c1[4] = {0x243F6A88u, 0x85A308D3u, 0x13198A2Eu, 0x03707344u}, k1[2] = {0xA4093822u, 0x299F31D0u};
        uint32_t out[4];
        fks_select_philox(c0, k0, out);
        CHECK(out[0] == 0x6627E8D5u && out[1] == 0xE169C58Du && out[2] == 0xBC57AC4Cu && out[3] == 0x9B00DBD8u);
        fks_select_philox(c1, k1, out);
        CHECK(out[0] == 0xD16CFE09u && out[1] == 0x94FDCCEBu && out[2] == 0x5001E420u && out[3] == 0x24126EA1u);
    }
}

int main() {
    test_refusals();
    test_invariants();
    test_twin();
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("select plan test ok\n");
    return 0;
}
