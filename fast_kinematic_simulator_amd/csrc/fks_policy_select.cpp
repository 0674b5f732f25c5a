/*
 * fks_policy_select.cpp — the selection of a policy table on the host (fks_policy_select): the
 * planner's single query during real execution (QueryBestAction) and the host twin of the policy
 * kernels' policy_select (fks_kernels.hip).
 *
 * Not the batch path (that is the GPU's, fks_forward_simulate_policy): it evaluates the same
 * expression trees as the kernel's ResetPosition at the start of a leg and its per-entry
 * configuration distance (config_distance<RT>, SPCS:898), with the shared portable libm and SE(3)
 * primitives (fks_portable_math.h, fks_se3.h; the host definitions are fks_host_distance.h's), so
 * the choices and distances of a roll-out equal this function's bit for bit.  No HIP, no context.
 */
#include <stddef.h>
#include <stdint.h>

#include <limits>
#include <vector>

#include "fks_capi.h"
#include "fks_host_distance.h"

using fks_host::config_distance;
using fks_host::reset_position;
using fks_host::weighted_dofs;
using fks_robot::Dof;

extern "C" fks_status fks_policy_select(const fks_robot_desc* robot, const fks_policy_table* table, const double* configs, uint64_t n,
                                        uint32_t* out_choice, double* out_distance) {
    std::vector<Dof> dofs;
    int W = 0;
    const fks_status st = weighted_dofs(robot, &dofs, &W);
    if (st != FKS_OK) return st;
    if (!table || !table->keys || !table->targets || table->num_entries == 0 || table->num_entries > FKS_MAX_POLICY_ENTRIES)
        return FKS_ERR_INVALID_ARGUMENT;
    if (table->terminal_distance != table->terminal_distance || table->max_distance != table->max_distance)
        return FKS_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!configs || !out_choice)) return FKS_ERR_INVALID_ARGUMENT;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> p((size_t)W);
    for (uint64_t c = 0; c < n; ++c) {
        reset_position(robot, dofs, W, configs + c * (uint64_t)W, p.data());
        /* strict < from +inf in ascending i: the lowest index wins a tie, a NaN never wins */
        double best = inf;
        uint32_t choice = FKS_POLICY_LOST;
        for (uint64_t i = 0; i < table->num_entries; ++i) {
            const double d = config_distance(robot, dofs, p.data(), table->keys + i * (uint64_t)W);
            if (d < best) {
                best = d;
                choice = (uint32_t)i;
            }
        }
        /* the lost test comes first */
        if (choice != FKS_POLICY_LOST) {
            if (best > table->max_distance)
                choice = FKS_POLICY_LOST;
            else if (table->flags && (table->flags[choice] & FKS_POLICY_ENTRY_TERMINAL) && best < table->terminal_distance)
                choice |= FKS_POLICY_ARRIVED;
        }
        out_choice[c] = choice;
        if (out_distance) out_distance[c] = best;
    }
    return FKS_OK;
}
