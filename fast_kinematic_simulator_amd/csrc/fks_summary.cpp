/*
 * fks_summary.cpp — fks_summarize_clusters: every cluster of every group made into a child state
 * (regrouped members, expectation, variances, the share within reach of a target) on the host; the
 * twin of the summary kernels (summarize_groups in fks_kernels.hip), which equal it byte for byte.
 *
 * The distance, the wrap and the SE(3) primitives are fks_host_distance.h's and fks_se3.h's, the
 * rotation mean fks_rotation_mean.h's; every sum runs over a cluster's members in ascending index
 * from +0.0, as fks_capi.h states.  No HIP, no context.
 */
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "fks_batch.h"
#include "fks_capi.h"
#include "fks_host_distance.h"
#include "fks_rotation_mean.h"

namespace {

/* a component whose mean is circular: a continuous dof, the SE(2) angle */
bool circular(const fks_robot_desc* robot, const std::vector<fks_robot::Dof>& dofs, size_t k) {
    if (robot->robot_type == FKS_ROBOT_LINKED) return dofs[k].type == FKS_JOINT_CONTINUOUS;
    return robot->robot_type == FKS_ROBOT_SE2 && k == 2;
}

}  // namespace

extern "C" fks_status fks_summarize_clusters(const fks_robot_desc* robot, const double* configs, const uint64_t* group_begin,
                                             uint64_t num_groups, const uint32_t* labels, const double* targets,
                                             double reached_distance, const fks_cluster_summary* out) {
    std::vector<fks_robot::Dof> dofs;
    int width = 0;
    fks_status st = fks_host::weighted_dofs(robot, &dofs, &width);
    if (st != FKS_OK) return st;
    fks_batch::SummaryPlan plan;
    std::string why;
    st = fks_batch::plan_summary(&plan, robot->robot_type, (uint32_t)width, configs, group_begin, num_groups, labels, targets,
                                 reached_distance, out, &why);
    if (st != FKS_OK) return st;
    const size_t W = (size_t)width, Wv = plan.var_width;
    const bool se3 = robot->robot_type == FKS_ROBOT_SE3;
    /* the passes whose outputs are all NULL are not run, as in the kernels */
    const bool want_mean = out->expectation || out->variances || out->variance;
    const bool want_spread = out->variances || out->variance;
    std::vector<uint32_t> count, begin, order, fill;
    std::vector<double> E(W), d2(Wv);
    for (uint64_t g = 0; g < num_groups; ++g) {
        const size_t first = (size_t)group_begin[g], n = (size_t)(group_begin[g + 1] - group_begin[g]);
        const uint32_t* lab = labels + first;
        /* the stable regrouping: a histogram, its exclusive prefix, then the members in ascending index */
        count.assign(n, 0);
        begin.assign(n, 0);
        order.assign(n, 0);
        for (size_t i = 0; i < n; ++i)
            if (lab[i] < n) ++count[lab[i]];
        uint32_t placed = 0;
        for (size_t c = 0; c < n; ++c) {
            begin[c] = placed;
            placed += count[c];
        }
        fill = begin;
        for (size_t i = 0; i < n; ++i) order[lab[i] < n ? fill[lab[i]]++ : placed++] = (uint32_t)i;
        for (size_t k = 0; k < n; ++k) {
            if (out->order) out->order[first + k] = (uint32_t)(first + order[k]);
            if (out->members)
                for (size_t w = 0; w < W; ++w) out->members[(first + k) * W + w] = configs[(first + order[k]) * W + w];
        }
        for (size_t c = 0; c < n; ++c) {
            const size_t r = first + c;
            const uint32_t m = count[c];
            const uint32_t* mem = order.data() + begin[c];
            if (out->count) out->count[r] = m;
            if (out->begin) out->begin[r] = (uint32_t)(first + begin[c]);
            const double dm = (double)m;
            double var = 0.0;
            uint32_t reached = 0;
            for (size_t w = 0; w < W; ++w) E[w] = 0.0;
            for (size_t w = 0; w < Wv; ++w) d2[w] = 0.0;
            if (m > 0 && want_mean) {
                if (se3) {
                    double S[fks_rotmean::kProducts], tx = 0.0, ty = 0.0, tz = 0.0, q[4], p[fks_rotmean::kProducts];
                    for (int a = 0; a < fks_rotmean::kProducts; ++a) S[a] = 0.0;
                    for (uint32_t j = 0; j < m; ++j) {
                        const double* c_i = configs + (first + mem[j]) * W;
                        fks_rotmean::quat_of_rotation34(c_i, q);
                        fks_rotmean::quat_products(q, p);
                        for (int a = 0; a < fks_rotmean::kProducts; ++a) S[a] = S[a] + p[a];
                        tx = tx + c_i[3];
                        ty = ty + c_i[7];
                        tz = tz + c_i[11];
                    }
                    fks_rotmean::dominant_eigenvector4(S, q);
                    fks_rotmean::rotation34_of_quat(q, E.data());
                    E[3] = tx / dm;
                    E[7] = ty / dm;
                    E[11] = tz / dm;
                } else {
                    for (size_t w = 0; w < W; ++w) {
                        if (circular(robot, dofs, w)) {
                            double ss = 0.0, sc = 0.0;
                            for (uint32_t j = 0; j < m; ++j) {
                                const double a = configs[(first + mem[j]) * W + w];
                                ss = ss + fks_math::sin(a);
                                sc = sc + fks_math::cos(a);
                            }
                            E[w] = fks_math::atan2(ss, sc);
                        } else {
                            double s = 0.0;
                            for (uint32_t j = 0; j < m; ++j) s = s + configs[(first + mem[j]) * W + w];
                            E[w] = s / dm;
                        }
                    }
                }
            }
            if (m > 0 && want_spread) {
                /* the second pass: differences from the expectation to each member */
                for (uint32_t j = 0; j < m; ++j) {
                    const double* c_i = configs + (first + mem[j]) * W;
                    if (se3) {
                        double Ei[12], Dm[12], tw[6];
                        fks_se3::inverse34(E.data(), Ei);
                        fks_se3::compose34(Ei, c_i, Dm);
                        fks_se3::log_twist34(Dm, tw);
                        for (size_t w = 0; w < 6; ++w) d2[w] = d2[w] + tw[w] * tw[w];
                    } else {
                        for (size_t w = 0; w < W; ++w) {
                            const double d = circular(robot, dofs, w) ? fks_math::wrap_revolute(c_i[w] - E[w]) : c_i[w] - E[w];
                            d2[w] = d2[w] + d * d;
                        }
                    }
                    const double dist = fks_host::config_distance(robot, dofs, E.data(), c_i);
                    var = var + dist * dist;
                }
                for (size_t w = 0; w < Wv; ++w) d2[w] = d2[w] / dm;
                var = var / dm;
            }
            if (targets)
                for (uint32_t j = 0; j < m; ++j) {
                    const double* c_i = configs + (first + mem[j]) * W;
                    if (fks_host::config_distance(robot, dofs, c_i, targets + g * W) < reached_distance) ++reached;
                }
            if (out->expectation)
                for (size_t w = 0; w < W; ++w) out->expectation[r * W + w] = E[w];
            if (out->variances)
                for (size_t w = 0; w < Wv; ++w) out->variances[r * Wv + w] = d2[w];
            if (out->variance) out->variance[r] = var;
            if (out->reached) out->reached[r] = reached;
        }
    }
    return FKS_OK;
}
