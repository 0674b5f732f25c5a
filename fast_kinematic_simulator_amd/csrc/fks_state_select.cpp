/*
 * fks_state_select.cpp — fks_select_states: for every query the nearest state of a table under a
 * per-state weight, and the draw of the chosen state's members into a job's starts, on the host;
 * the twin of the selection kernels (fks_state_select_<family> and fks_state_draw in
 * fks_kernels.hip), which equal it byte for byte.
 *
 * The distance is fks_host_distance.h's; the draw is integer arithmetic over a Philox4x32-10 of
 * this file's own (the statement is in fks_capi.h).  No HIP, no context.
 */
#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "fks_batch.h"
#include "fks_capi.h"
#include "fks_host_distance.h"

namespace {

uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

/* Philox4x32-10 (Salmon et al., Random123): ten rounds, the key bumped by the Weyl constants */
void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(M0, c[0]), lo0 = M0 * c[0];
        const uint32_t hi1 = mulhi32(M1, c[2]), lo1 = M1 * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += W0;
        k1 += W1;
    }
}

/* member r_k * c >> 32 of job j's start k */
uint32_t drawn_member(uint64_t j, uint32_t k, uint32_t c, uint32_t k0, uint32_t k1) {
    uint32_t ctr[4] = {(uint32_t)j, k >> 2, (uint32_t)(j >> 32), 0x44524157u};
    philox4x32_10(ctr, k0, k1);
    return (uint32_t)(((uint64_t)ctr[k & 3u] * (uint64_t)c) >> 32);
}

}  // namespace

extern "C" void fks_select_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
    philox4x32_10(c, key[0], key[1]);
    for (int k = 0; k < 4; ++k) out[k] = c[k];
}

extern "C" fks_status fks_select_states_plan(uint64_t num_queries, uint64_t num_states, int32_t compute_units, uint64_t out[4]) {
    if (!out) return FKS_ERR_INVALID_ARGUMENT;
    fks_state_table t;
    std::memset(&t, 0, sizeof(t));
    double key = 0.0; /* never dereferenced */
    uint32_t word = 0;
    t.keys = &key;
    t.num_states = num_states;
    fks_state_selection s;
    std::memset(&s, 0, sizeof(s));
    s.choice = &word;
    fks_batch::SelectPlan plan;
    std::string why;
    const fks_status st = fks_batch::plan_select(&plan, 1, compute_units, &t, &key, num_queries, 0, &s, &why);
    if (st != FKS_OK) return st;
    out[0] = plan.tile;
    out[1] = plan.chunk_states;
    out[2] = plan.chunks;
    out[3] = plan.groups;
    return FKS_OK;
}

extern "C" fks_status fks_select_states(const fks_robot_desc* robot, const fks_state_table* table, const double* queries,
                                        uint64_t num_queries, uint32_t num_particles, uint64_t draw_seed, const fks_state_selection* out) {
    std::vector<fks_robot::Dof> dofs;
    int width = 0;
    fks_status st = fks_host::weighted_dofs(robot, &dofs, &width);
    if (st != FKS_OK) return st;
    fks_batch::SelectPlan plan;
    std::string why;
    st = fks_batch::plan_select(&plan, (uint32_t)width, 1, table, queries, num_queries, num_particles, out, &why);
    if (st != FKS_OK) return st;
    const size_t W = (size_t)width, P = num_particles;
    const uint64_t S = table->num_states;
    const uint64_t key = fks_batch::splitmix64(draw_seed);
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const double inf = std::numeric_limits<double>::infinity();
    for (uint64_t j = 0; j < num_queries; ++j) {
        const double* q = queries + j * W;
        /* strict < from +inf in ascending i: the lowest index wins a tie, a NaN never wins */
        double best = inf;
        uint32_t choice = FKS_STATE_NONE;
        for (uint64_t i = 0; i < S; ++i) {
            if (table->count && table->count[i] == 0) continue;
            double d = fks_host::config_distance(robot, dofs, table->keys + i * W, q);
            if (table->weights) d = table->weights[i] * d;
            if (d < best) {
                best = d;
                choice = (uint32_t)i;
            }
        }
        out->choice[j] = choice;
        if (out->distance) out->distance[j] = best;
        if (!plan.draw) continue;
        uint32_t* src = out->source ? out->source + j * P : nullptr;
        double* rows = out->starts ? out->starts + j * P * W : nullptr;
        const uint64_t c = choice != FKS_STATE_NONE ? table->count[choice] : 0;
        const uint64_t b = choice != FKS_STATE_NONE ? table->begin[choice] : 0;
        const bool none = choice == FKS_STATE_NONE || b + c > table->num_member_rows;
        for (size_t k = 0; k < P; ++k) {
            if (none) {
                if (src) src[k] = FKS_STATE_NONE;
                if (rows)
                    for (size_t w = 0; w < W; ++w) rows[k * W + w] = 0.0;
                continue;
            }
            /* below b + c <= num_member_rows; a begin is a uint32, so a summary's pool has no row past 2^32 */
            const uint64_t row = b + (c == P ? (uint64_t)k : (uint64_t)drawn_member(j, (uint32_t)k, (uint32_t)c, k0, k1));
            if (src) src[k] = (uint32_t)row;
            if (rows) std::memcpy(rows + k * W, table->members + (size_t)row * W, W * sizeof(double));
        }
    }
    return FKS_OK;
}
