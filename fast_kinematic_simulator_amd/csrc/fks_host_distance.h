/*
 * fks_host_distance.h — the robot's ResetPosition and configuration distance on the host,
 * read from an fks_robot_desc: the one host definition behind fks_policy_select
 * (fks_policy_select.cpp) and fks_cluster_configs (fks_cluster.cpp).
 *
 * The same expression trees as the kernels' reset and config_distance_of<RT> (fks_kernels.hip),
 * over the shared portable libm and SE(3) primitives (fks_portable_math.h, fks_se3.h), so a value
 * computed here equals the device's bit for bit.  Internal: no HIP, no context.
 */
#ifndef FKS_HOST_DISTANCE_H
#define FKS_HOST_DISTANCE_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "fks_capi.h"
#include "fks_portable_math.h"
#include "fks_robot.h"
#include "fks_se3.h"

namespace fks_host {

using fks_math::clamp;
using fks_math::dabs;
using fks_math::dsqrt;

/* the dofs and width of a robot that has distance weights; FKS_ERR_INVALID_ARGUMENT for a malformed one */
inline fks_status weighted_dofs(const fks_robot_desc* d, std::vector<fks_robot::Dof>* dofs, int* width) {
    if (!d || !d->distance_weights) return FKS_ERR_INVALID_ARGUMENT;
    return fks_robot::dof_table(d, dofs, width);
}

/* ResetPosition(q) -> SetPosition: joint limits / angle wrap (the kernel's seg == 0 branch) */
inline void reset_position(const fks_robot_desc* robot, const std::vector<fks_robot::Dof>& dofs, int W, const double* q, double* p) {
    if (robot->robot_type == FKS_ROBOT_LINKED) {
        for (int k = 0; k < W; ++k)
            p[k] = dofs[(size_t)k].type == FKS_JOINT_CONTINUOUS ? fks_math::wrap_revolute(q[k])
                                                                : clamp(q[k], dofs[(size_t)k].lo, dofs[(size_t)k].hi);
    } else if (robot->robot_type == FKS_ROBOT_SE2) {
        p[0] = q[0];
        p[1] = q[1];
        p[2] = fks_math::wrap_revolute(q[2]);
    } else {
        for (int k = 0; k < 12; ++k) p[k] = q[k];
    }
}

/* ComputeConfigurationDistanceTo: config_distance_of<RT> of fks_kernels.hip from cfg to target */
inline double config_distance(const fks_robot_desc* robot, const std::vector<fks_robot::Dof>& dofs, const double* cfg, const double* target) {
    const double* w = robot->distance_weights;
    if (robot->robot_type == FKS_ROBOT_LINKED) {
        double sum = 0.0;
        for (size_t k = 0; k < dofs.size(); ++k) {
            const double sd = dofs[k].type == FKS_JOINT_CONTINUOUS ? fks_math::wrap_revolute(target[k] - cfg[k]) : target[k] - cfg[k];
            const double d = w[k] * dabs(sd);
            sum = sum + d * d;
        }
        return dsqrt(sum);
    }
    if (robot->robot_type == FKS_ROBOT_SE2) {
        const double dx = target[0] - cfg[0];
        const double dy = target[1] - cfg[1];
        const double dr = fks_math::wrap_revolute(target[2] - cfg[2]);
        return w[0] * dsqrt(dx * dx + dy * dy) + w[1] * dabs(dr);
    }
    double Pi[12], Dm[12], tw[6];
    const double dx = target[3] - cfg[3], dy = target[7] - cfg[7], dz = target[11] - cfg[11];
    fks_se3::inverse34(cfg, Pi);
    fks_se3::compose34(Pi, target, Dm);
    fks_se3::log_twist34(Dm, tw);
    const double angle = dsqrt((tw[3] * tw[3] + tw[4] * tw[4]) + tw[5] * tw[5]);
    return w[0] * dsqrt((dx * dx + dy * dy) + dz * dz) + w[1] * angle;
}

}  // namespace fks_host

#endif
