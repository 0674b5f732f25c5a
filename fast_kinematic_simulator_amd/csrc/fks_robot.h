/*
 * fks_robot.h — the host half of a robot: the checks of an fks_robot_desc that arrives from
 * outside the library, its dof numbering, the kernels' tables flattened from it, and the
 * constants the skip proofs rest on: the per-dof levers and per-round
 * radii of the robot, the Lipschitz-type constants of the environment's SDF.
 *
 * Nothing here calls the HIP runtime or reads an fks_context: fks_set_robot uploads what flatten
 * fills, fks_create reads what analyze_sdf returns, so the unit is built and tested on a machine
 * without a GPU (tests/cpp/robot_flatten_test.cpp).
 */
#ifndef FKS_ROBOT_H
#define FKS_ROBOT_H

#include <hip/hip_vector_types.h> /* the vector types fks_device.h names */
#include <stdint.h>

#include <string>
#include <vector>

#include "fks_capi.h"
#include "fks_device.h"

namespace fks_robot {

/* one degree of freedom of a linked robot: its joint's index, type and limits */
struct Dof {
    int32_t joint;
    int32_t type;
    double lo, hi;
};

/* The robot's dofs and its flat configuration width: a linked robot's non-fixed joints in joint
 * order (width num_dofs); none for SE(2) (3 dofs, width 3) and SE(3) (6 dofs, width 12).  The one
 * definition of the numbering: the kernels' tables (flatten), the control twins
 * (fks_robot_control.cpp) and the host distance (fks_host_distance.h) all read it here.
 * FKS_ERR_INVALID_ARGUMENT for a null description, joints that are missing, a num_dofs that is
 * not the number of non-fixed joints (>= 1) or not 3 / 6, and an unknown robot type. */
fks_status dof_table(const fks_robot_desc* d, std::vector<Dof>* dofs, int* width);

/* a description flattened into the kernels' tables: what fks_set_robot uploads, one array each */
struct Flat {
    fksd::RobotDev R; /* type, L, J, G, D, P, W, npairs, self_possible, nrounds, base; every pointer null */
    std::vector<fksd::JointDev> joints;
    std::vector<int32_t> dof_joint;
    std::vector<uint64_t> link_dof_mask;
    std::vector<uint16_t> point_geom, point_link;
    std::vector<double> geom_box;  /* 7 per geometry */
    std::vector<double> geom_mass;
    std::vector<uint64_t> allowed_mask;
    std::vector<int32_t> pairs;    /* 2 per disallowed pair */
    std::vector<fksd::RoundDev> rounds;             /* max(1, nrounds) */
    std::vector<double> dof_lever, dof_lever_box;   /* max(1, D) */
    std::vector<double> weights;
};

/* Checks `d` (not null) and fills `out`.  A refusal returns its status with the text in `why`
 * and leaves `out` unspecified. */
fks_status flatten(const fks_robot_desc* d, Flat* out, std::string* why);

/* Lipschitz-type constants of the SDF that make a round of points provably free of
 * contact: over axis-neighbour cell pairs, lplus = max |a - b| / res
 * where both values are positive, cmax = max a / res over positive cells with a
 * non-positive neighbour.  For an exact signed EDT both are 1.  Any non-finite value
 * disables skipping (false, as does a field with no positive pair). */
bool analyze_sdf(const float* v, int64_t nx, int64_t ny, int64_t nz, double res, double* lplus, double* cmax);

}  // namespace fks_robot

#endif
