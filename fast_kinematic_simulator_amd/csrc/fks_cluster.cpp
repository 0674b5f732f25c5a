/*
 * fks_cluster.cpp — fks_cluster_configs: the configuration-distance matrices of G groups and their
 * complete-link clusters under a threshold, on the host; the twin of the clustering kernels
 * (cluster_groups in fks_kernels.hip), which equal it byte for byte.
 *
 * The distance is fks_host_distance.h's (the expression trees of config_distance_of<RT>); the
 * clustering is the definition in fks_capi.h: links are maxima of matrix entries, merged links are
 * max(L(a, k), L(b, k)), every comparison is on doubles that both sides hold bit for bit, so the
 * labels depend on the matrix's bits alone.  No HIP, no context.
 */
#include <stddef.h>
#include <stdint.h>

#include <limits>
#include <string>
#include <vector>

#include "fks_batch.h"
#include "fks_capi.h"
#include "fks_host_distance.h"

namespace {

/* complete link over the n x n matrix M (row-major; only i < j is read) */
void cluster_matrix(const double* M, uint32_t n, double threshold, uint32_t* labels, uint32_t* count) {
    const double inf = std::numeric_limits<double>::infinity();
    /* the working links: a distance that is not < +inf counts as +inf */
    std::vector<double> L((size_t)n * n);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i + 1; j < n; ++j) {
            const double d = M[(size_t)i * n + j];
            L[(size_t)i * n + j] = (d < inf) ? d : inf;
        }
    std::vector<uint8_t> alive(n, 1);
    std::vector<uint32_t> name(n); /* a configuration's cluster: its smallest member */
    for (uint32_t i = 0; i < n; ++i) name[i] = i;
    for (;;) {
        /* ascending (a, b) under a strict < from +inf: the lowest pair wins a tie, +inf never wins */
        double best = inf;
        uint32_t ba = 0, bb = 0;
        bool found = false;
        for (uint32_t a = 0; a < n; ++a) {
            if (!alive[a]) continue;
            for (uint32_t b = a + 1; b < n; ++b) {
                if (!alive[b]) continue;
                const double l = L[(size_t)a * n + b];
                if (l < best) {
                    best = l;
                    ba = a;
                    bb = b;
                    found = true;
                }
            }
        }
        if (!found || best > threshold) break;
        /* b joins a: L(a u b, k) = max(L(a, k), L(b, k)) */
        for (uint32_t k = 0; k < n; ++k) {
            if (!alive[k] || k == ba || k == bb) continue;
            double& lak = (k < ba) ? L[(size_t)k * n + ba] : L[(size_t)ba * n + k];
            const double lbk = (k < bb) ? L[(size_t)k * n + bb] : L[(size_t)bb * n + k];
            lak = (lbk > lak) ? lbk : lak;
        }
        alive[bb] = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (name[i] == bb) name[i] = ba;
    }
    /* numbered in ascending order of the smallest member */
    std::vector<uint32_t> number(n, 0);
    uint32_t c = 0;
    for (uint32_t k = 0; k < n; ++k)
        if (alive[k]) number[k] = c++;
    if (labels)
        for (uint32_t i = 0; i < n; ++i) labels[i] = number[name[i]];
    *count = c;
}

}  // namespace

extern "C" fks_status fks_cluster_configs(const fks_robot_desc* robot, const double* configs, const uint64_t* group_begin,
                                          uint64_t num_groups, double threshold, double* out_distances, uint32_t* out_labels,
                                          uint32_t* out_num_clusters) {
    std::vector<fks_robot::Dof> dofs;
    int W = 0;
    fks_status st = fks_host::weighted_dofs(robot, &dofs, &W);
    if (st != FKS_OK) return st;
    fks_batch::ClusterPlan plan;
    std::string why;
    st = fks_batch::plan_cluster(&plan, configs, group_begin, num_groups, threshold, out_distances, out_labels, out_num_clusters, &why);
    if (st != FKS_OK) return st;
    std::vector<double> own; /* a group's matrix when the caller takes none */
    for (uint64_t g = 0; g < num_groups; ++g) {
        const uint64_t first = group_begin[g], n = group_begin[g + 1] - first;
        double* M = out_distances ? out_distances + plan.mat_begin[(size_t)g] : nullptr;
        if (!M) {
            own.resize((size_t)(n * n));
            M = own.data();
        }
        for (uint64_t i = 0; i < n; ++i) {
            M[i * n + i] = 0.0;
            for (uint64_t j = i + 1; j < n; ++j) {
                /* cfg = c_i, target = c_j; the lower triangle is the same bits, never c_j -> c_i */
                const double d = fks_host::config_distance(robot, dofs, configs + (first + i) * (uint64_t)W, configs + (first + j) * (uint64_t)W);
                M[i * n + j] = d;
                M[j * n + i] = d;
            }
        }
        if (plan.labelled) {
            uint32_t count = 0;
            cluster_matrix(M, (uint32_t)n, threshold, out_labels ? out_labels + first : nullptr, &count);
            if (out_num_clusters) out_num_clusters[g] = count;
        }
    }
    return FKS_OK;
}
