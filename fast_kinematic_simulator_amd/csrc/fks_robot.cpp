/*
 * fks_robot.cpp — see fks_robot.h.  No HIP runtime call, no context.
 */
#include "fks_robot.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

namespace fks_robot {

using fksd::JointDev;
using fksd::RobotDev;

fks_status dof_table(const fks_robot_desc* d, std::vector<Dof>* dofs, int* width) {
    if (!d) return FKS_ERR_INVALID_ARGUMENT;
    dofs->clear();
    if (d->robot_type == FKS_ROBOT_LINKED) {
        if (d->num_joints < 0 || (d->num_joints > 0 && !d->joints)) return FKS_ERR_INVALID_ARGUMENT;
        for (int32_t j = 0; j < d->num_joints; ++j) {
            const fks_joint_desc& jd = d->joints[j];
            if (jd.type == FKS_JOINT_FIXED) continue;
            dofs->push_back(Dof{j, jd.type, jd.limit_lower, jd.limit_upper});
        }
        if ((int32_t)dofs->size() != d->num_dofs || d->num_dofs < 1) return FKS_ERR_INVALID_ARGUMENT;
        *width = d->num_dofs;
        return FKS_OK;
    }
    if (d->robot_type == FKS_ROBOT_SE2 && d->num_dofs == 3) {
        *width = 3;
        return FKS_OK;
    }
    if (d->robot_type == FKS_ROBOT_SE3 && d->num_dofs == 6) {
        *width = 12;
        return FKS_OK;
    }
    return FKS_ERR_INVALID_ARGUMENT;
}

fks_status flatten(const fks_robot_desc* d, Flat* out, std::string* why) {
    auto refuse = [&](const char* text) {
        *why = text;
        return FKS_ERR_INVALID_ARGUMENT;
    };
    const int G = d->num_geometries;
    if (G < 1 || G > fksd::kMaxGeoms || !d->geometry_link || !d->geometry_point_offset || !d->points || !d->controllers)
        return refuse("robot geometries/controllers missing or more than 64 geometries");
    const uint32_t P = d->geometry_point_offset[G];
    if (d->geometry_point_offset[0] != 0 || P < 1 || P > 65535) return refuse("robot needs 1..65535 points with offsets starting at 0");
    for (int g = 0; g < G; ++g)
        if (d->geometry_point_offset[g + 1] < d->geometry_point_offset[g]) return refuse("geometry offsets must be non-decreasing");
    for (uint32_t i = 0; i < 4 * P; ++i)
        if (!std::isfinite(d->points[i])) return refuse("non-finite robot point");
    *out = Flat();
    RobotDev& R = out->R;
    std::memset(&R, 0, sizeof(R));
    R.type = d->robot_type;
    R.G = G;
    R.P = (int32_t)P;
    std::vector<JointDev>& joints = out->joints;
    std::vector<int32_t>& dof_joint = out->dof_joint;
    std::vector<int32_t> link_parent_joint;
    if (d->robot_type == FKS_ROBOT_LINKED) {
        const int L = d->num_links, J = d->num_joints;
        if (L < 1 || L > fksd::kMaxLinks || J < 0 || J > fksd::kMaxJoints || (J > 0 && !d->joints))
            return refuse("linked robot needs 1..64 links and 0..64 joints");
        std::vector<int> seen(L, 0);
        seen[0] = 1;
        link_parent_joint.assign(L, -1);
        for (int j = 0; j < J; ++j) {
            const fks_joint_desc& jd = d->joints[j];
            if (jd.parent_link < 0 || jd.parent_link >= L || jd.child_link <= 0 || jd.child_link >= L)
                return refuse("joint link index out of range");
            if (!seen[jd.parent_link] || seen[jd.child_link]) return refuse("joints must be in topological order, one parent per link");
            seen[jd.child_link] = 1;
            link_parent_joint[jd.child_link] = j;
            if (jd.type != FKS_JOINT_FIXED && jd.type != FKS_JOINT_REVOLUTE && jd.type != FKS_JOINT_CONTINUOUS &&
                jd.type != FKS_JOINT_PRISMATIC)
                return refuse("unknown joint type");
            JointDev jv;
            std::memset(&jv, 0, sizeof(jv));
            jv.parent = jd.parent_link;
            jv.child = jd.child_link;
            jv.type = jd.type;
            jv.dof = -1;
            std::memcpy(jv.origin, jd.origin, sizeof(jv.origin));
            std::memcpy(jv.axis, jd.axis, sizeof(jv.axis));
            jv.lo = jd.limit_lower;
            jv.hi = jd.limit_upper;
            joints.push_back(jv);
        }
        for (int l = 0; l < L; ++l)
            if (!seen[l]) return refuse("every link must be reached by a joint");
        std::vector<Dof> dofs;
        int W = 0;
        if (dof_table(d, &dofs, &W) != FKS_OK || d->num_dofs > fksd::kMaxDofs)
            return refuse("num_dofs must equal the number of non-fixed joints (1..64)");
        for (const Dof& dof : dofs) {
            joints[dof.joint].dof = (int32_t)dof_joint.size();
            dof_joint.push_back(dof.joint);
        }
        for (int g = 0; g < G; ++g)
            if (d->geometry_link[g] < 0 || d->geometry_link[g] >= L) return refuse("geometry link index out of range");
        R.L = L;
        R.J = J;
        R.D = d->num_dofs;
        R.W = W;
    } else if (d->robot_type == FKS_ROBOT_SE2 || d->robot_type == FKS_ROBOT_SE3) {
        std::vector<Dof> dofs;
        int W = 0;
        if (dof_table(d, &dofs, &W) != FKS_OK || G != 1 || d->geometry_link[0] != 0)
            return refuse("SE(2)/SE(3) robots have one geometry on link 0 and 3/6 dofs");
        R.L = 1;
        R.J = 0;
        R.D = d->num_dofs;
        R.W = W;
    } else {
        return refuse("unknown robot type");
    }
    std::memcpy(R.base, d->base_transform, sizeof(R.base));
    /* allowed self-collision masks (CheckIfSelfCollisionAllowed, symmetric, self allowed) */
    std::vector<uint64_t>& allowed = out->allowed_mask;
    allowed.assign(G, 0);
    for (int g = 0; g < G; ++g) allowed[g] |= 1ull << g;
    for (int k = 0; k < d->num_allowed_pairs; ++k) {
        const int a = d->allowed_pairs[2 * k], b = d->allowed_pairs[2 * k + 1];
        if (a < 0 || a >= G || b < 0 || b >= G) return refuse("allowed pair out of range");
        allowed[a] |= 1ull << b;
        allowed[b] |= 1ull << a;
    }
    std::vector<int32_t>& pairs = out->pairs;
    for (int a = 0; a < G; ++a)
        for (int b = a + 1; b < G; ++b)
            if (!((allowed[a] >> b) & 1ull)) {
                pairs.push_back(a);
                pairs.push_back(b);
            }
    R.npairs = (int32_t)(pairs.size() / 2);
    R.self_possible = !(G == 1 || (G == 2 && ((allowed[0] >> 1) & 1ull)));
    /* per point geometry, per geometry local boxes and link masses (SPCS:1244-1255) */
    std::vector<uint16_t>& point_geom = out->point_geom;
    std::vector<uint16_t>& point_link = out->point_link;
    point_geom.assign(P, 0);
    point_link.assign(P, 0);
    std::vector<double>& box = out->geom_box;
    std::vector<double>& mass = out->geom_mass;
    box.assign(7 * (size_t)G, 0.0);
    mass.assign(G, 0.0);
    for (int g = 0; g < G; ++g) {
        const uint32_t b0 = d->geometry_point_offset[g], b1 = d->geometry_point_offset[g + 1];
        double mn[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, mx[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        bool w_one = true;
        for (uint32_t i = b0; i < b1; ++i) {
            point_geom[i] = (uint16_t)g;
            point_link[i] = (uint16_t)d->geometry_link[g];
            for (int a = 0; a < 3; ++a) {
                mn[a] = std::fmin(mn[a], d->points[4 * i + a]);
                mx[a] = std::fmax(mx[a], d->points[4 * i + a]);
            }
            w_one = w_one && d->points[4 * i + 3] == 1.0;
        }
        if (b1 == b0) {
            for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0;
        }
        for (int a = 0; a < 3; ++a) {
            box[7 * g + a] = 0.5 * (mn[a] + mx[a]);
            box[7 * g + 3 + a] = 0.5 * (mx[a] - mn[a]);
        }
        box[7 * g + 6] = w_one ? 1.0 : 0.0;
    }
    /* 64-point rounds of the kernel's lane-strided loops */
    const int NR = ((int)P + 63) / 64;
    std::vector<fksd::RoundDev>& rounds = out->rounds;
    rounds.resize(NR > 0 ? NR : 1);
    for (int r = 0; r < NR; ++r) {
        fksd::RoundDev rd;
        rd.link = -1;
        rd.npts = std::min(64, (int)P - 64 * r);
        rd.radius = 0.0;
        bool uniform = true;
        for (int i = 64 * r; i < 64 * r + rd.npts; ++i) {
            const double* p = d->points + 4 * (size_t)i;
            uniform = uniform && point_link[i] == point_link[64 * r] && p[3] == 1.0;
            rd.radius = std::max(rd.radius, std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
        }
        if (uniform && std::isfinite(rd.radius)) rd.link = point_link[64 * r];
        rd.radius = rd.radius * (1.0 + 1e-9) + 1e-12;
        rounds[r] = rd;
    }
    R.nrounds = NR;
    double previous_link_masses = 0.0;
    for (int g = G - 1; g >= 0; --g) {
        const double link_mass = (double)(d->geometry_point_offset[g + 1] - d->geometry_point_offset[g]);
        mass[g] = link_mass + previous_link_masses;
        previous_link_masses += link_mass;
    }
    /* dofs moving each link: joints whose child is an ancestor-or-self of the link */
    std::vector<uint64_t>& link_mask = out->link_dof_mask;
    link_mask.assign(R.L, 0);
    if (d->robot_type == FKS_ROBOT_LINKED) {
        for (int l = 0; l < R.L; ++l) {
            int cur = l;
            while (cur > 0) {
                const int j = link_parent_joint[cur];
                if (joints[j].dof >= 0) link_mask[l] |= 1ull << joints[j].dof;
                cur = joints[j].parent;
            }
        }
    }
    /* reach from joint jd's frame origin (= its child link origin) down to link l, a link that
     * jd moves: the origin offsets of the joints on the path; prismatic joints on it add their
     * largest stroke */
    auto reach_from = [&](int jd, int l) {
        double reach = 0.0;
        for (int cur = l; cur != joints[jd].child;) {
            const JointDev& jp = joints[link_parent_joint[cur]];
            reach += std::sqrt(jp.origin[3] * jp.origin[3] + jp.origin[7] * jp.origin[7] + jp.origin[11] * jp.origin[11]);
            if (jp.type == FKS_JOINT_PRISMATIC)
                reach += std::max(std::fabs(jp.lo), std::fabs(jp.hi)) *
                         std::sqrt(jp.axis[0] * jp.axis[0] + jp.axis[1] * jp.axis[1] + jp.axis[2] * jp.axis[2]);
            cur = jp.parent;
        }
        return reach;
    };
    /* lever arm bound per dof: max over downstream points of (path reach from the
     * joint frame origin) + |p| */
    std::vector<double>& lever = out->dof_lever;
    lever.assign(std::max(1, R.D), HUGE_VAL);
    if (d->robot_type == FKS_ROBOT_LINKED) {
        bool w_one = true;
        for (uint32_t i = 0; i < P; ++i) w_one = w_one && d->points[4 * (size_t)i + 3] == 1.0;
        for (int k = 0; k < R.D && w_one; ++k) {
            const int jd = dof_joint[k];
            if (joints[jd].type == FKS_JOINT_PRISMATIC) {
                const double* ax = joints[jd].axis;
                lever[k] = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
                continue;
            }
            double worst = 0.0;
            for (int g = 0; g < G; ++g) {
                const int l = d->geometry_link[g];
                if (!((link_mask[l] >> k) & 1ull)) continue;
                const double reach = reach_from(jd, l);
                for (uint32_t i = d->geometry_point_offset[g]; i < d->geometry_point_offset[g + 1]; ++i) {
                    const double* p = d->points + 4 * (size_t)i;
                    worst = std::max(worst, reach + std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
                }
            }
            const double* ax = joints[jd].axis;
            const double an = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
            /* AngleAxis with a non-unit axis is not a rotation: no bound */
            lever[k] = (std::fabs(an - 1.0) < 1e-12 && std::isfinite(worst)) ? worst * (1.0 + 1e-9) + 1e-12 : HUGE_VAL;
        }
    } else {
        /* SE(2) (x, y, theta, applied additively) and SE(3) (body twist v, w: P * exp(twist)):
         * a point p of the body moves by at most |dt| + |rotation angle| * |p|, the angle at most
         * the sum of the angular components' magnitudes and |V v| <= |v| (exp's V has operator
         * norm <= 1), so translation components get lever 1, rotation components max |p| */
        bool w_one = true;
        double rmax = 0.0;
        for (uint32_t i = 0; i < P; ++i) {
            const double* p = d->points + 4 * (size_t)i;
            w_one = w_one && p[3] == 1.0;
            rmax = std::max(rmax, std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
        }
        if (w_one && std::isfinite(rmax)) {
            const int nt = d->robot_type == FKS_ROBOT_SE2 ? 2 : 3; /* translation components first */
            for (int k = 0; k < R.D; ++k) lever[k] = (k < nt) ? 1.0 + 1e-9 : rmax * (1.0 + 1e-9) + 1e-12;
        }
    }
    /* the same bound over the geometries' local boxes (corner distance <= |centre| + |half
     * extents|): the self-collision boxes are built from them */
    std::vector<double>& lever_box = out->dof_lever_box;
    lever_box.assign(std::max(1, R.D), HUGE_VAL);
    if (d->robot_type == FKS_ROBOT_LINKED) {
        for (int k = 0; k < R.D; ++k) {
            const int jd = dof_joint[k];
            if (joints[jd].type == FKS_JOINT_PRISMATIC) {
                lever_box[k] = lever[k];
                continue;
            }
            const double* ax = joints[jd].axis;
            const double an = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
            double worst = 0.0;
            bool ok = std::fabs(an - 1.0) < 1e-12;
            for (int g = 0; g < G && ok; ++g) {
                const int l = d->geometry_link[g];
                if (!((link_mask[l] >> k) & 1ull)) continue;
                const double* b = box.data() + 7 * (size_t)g;
                if (b[6] == 0.0) {
                    ok = false; /* no box (a point with w != 1): the box test never skips anyway */
                    break;
                }
                const double reach = reach_from(jd, l);
                worst = std::max(worst, reach + std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]) +
                                            std::sqrt(b[3] * b[3] + b[4] * b[4] + b[5] * b[5]));
            }
            lever_box[k] = (ok && std::isfinite(worst)) ? worst * (1.0 + 1e-9) + 1e-12 : HUGE_VAL;
        }
    }
    std::vector<double>& weights = out->weights;
    if (d->robot_type == FKS_ROBOT_LINKED) {
        for (int k = 0; k < R.D; ++k) weights.push_back(d->distance_weights ? d->distance_weights[k] : 1.0);
    } else {
        weights.push_back(d->distance_weights ? d->distance_weights[0] : 1.0);
        weights.push_back(d->distance_weights ? d->distance_weights[1] : 1.0);
    }
    /* SampledUncertainVelocityActuator tables (UNC:123-281) */
    if (d->sampled_actuators) {
        for (int k = 0; k < R.D; ++k) {
            const fks_sampled_actuator& a = d->sampled_actuators[k];
            if (a.num_bins == 0) continue;
            if (a.bin_elements == 0 || !a.bin_bounds || !a.bin_samples) return refuse("sampled actuator needs bounds and >= 1 sample per bin");
            for (uint64_t i = 0; i < 2ull * a.num_bins; ++i)
                if (std::isnan(a.bin_bounds[i])) return refuse("NaN sampled-actuator bin bound");
            for (uint64_t i = 0; i < (uint64_t)a.num_bins * a.bin_elements; ++i)
                if (!std::isfinite(a.bin_samples[i])) return refuse("non-finite sampled-actuator sample");
        }
    }
    return FKS_OK;
}

bool analyze_sdf(const float* v, int64_t nx, int64_t ny, int64_t nz, double res, double* lplus, double* cmax) {
    const int T = (int)std::max<unsigned>(1u, std::min<unsigned>(16u, std::thread::hardware_concurrency()));
    std::vector<double> lp(T, 0.0), cm(T, 0.0);
    std::vector<int> bad(T, 0);
    std::vector<std::thread> th;
    const double inv = 1.0 / res;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t]() {
            for (int64_t x = t; x < nx; x += T)
                for (int64_t y = 0; y < ny; ++y)
                    for (int64_t z = 0; z < nz; ++z) {
                        const size_t i = ((size_t)x * ny + y) * nz + z;
                        const double a = v[i];
                        if (!std::isfinite(a)) {
                            bad[t] = 1;
                            continue;
                        }
                        const size_t nb[3] = {x + 1 < nx ? i + (size_t)ny * nz : i, y + 1 < ny ? i + (size_t)nz : i,
                                              z + 1 < nz ? i + 1 : i};
                        for (int k = 0; k < 3; ++k) {
                            if (nb[k] == i) continue;
                            const double b = v[nb[k]];
                            if (!std::isfinite(b)) continue; /* flagged when visited */
                            if (a > 0.0 && b > 0.0) {
                                lp[t] = std::max(lp[t], std::fabs(a - b) * inv);
                            } else if (a > 0.0) {
                                cm[t] = std::max(cm[t], a * inv);
                            } else if (b > 0.0) {
                                cm[t] = std::max(cm[t], b * inv);
                            }
                        }
                    }
        });
    for (auto& h : th) h.join();
    *lplus = 0.0;
    *cmax = 0.0;
    for (int t = 0; t < T; ++t) {
        if (bad[t]) return false;
        *lplus = std::max(*lplus, lp[t]);
        *cmax = std::max(*cmax, cm[t]);
    }
    return *lplus > 0.0;
}

}  // namespace fks_robot
