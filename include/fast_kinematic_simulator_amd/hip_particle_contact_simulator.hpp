/*
 * hip_particle_contact_simulator.hpp — C++ host mirror of the reference
 * simulator interface over the C-ABI in fks_capi.h (header-only, C++17).
 *
 * Mirrors simple_particle_contact_simulator::SimpleParticleContactSimulator as the
 * planner sees it through uncertainty_planning_core's SimulatorInterface
 * (reference: include/fast_kinematic_simulator/simple_particle_contact_simulator.hpp,
 * "SPCS") and the factories of fast_kinematic_simulator.hpp/.cpp ("FKS").  Method
 * names, argument meaning and result layout follow the reference; configurations
 * are flat double vectors (linked robot: joint values; SE(2): x, y, theta;
 * SE(3): 3x4 row-major pose) because the reference's Eigen / arc_utilities types
 * are not part of this repository.  INTEGRATION.md shows the conversion a
 * maintainer adds on the reference side.
 *
 * Every simulation runs on the GPU through libfks_hip.so; there is no CPU
 * fallback.  Errors from the C-ABI are raised as fks::SimulatorError.
 */
#ifndef FAST_KINEMATIC_SIMULATOR_AMD_HIP_PARTICLE_CONTACT_SIMULATOR_HPP
#define FAST_KINEMATIC_SIMULATOR_AMD_HIP_PARTICLE_CONTACT_SIMULATOR_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <limits>
#include <random>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "fast_kinematic_simulator_amd/device_set.hpp"
#include "fks_capi.h"

namespace fks {

inline void check(fks_status st, const fks_context* ctx, const char* what) {
    if (st == FKS_OK) return;
    std::string msg = std::string(what) + ": " + fks_status_string(st);
    if (ctx) {
        const char* detail = fks_get_last_error(ctx);
        if (detail && detail[0]) msg += std::string(" (") + detail + ")";
    }
    throw SimulatorError(st, msg);
}

using Configuration = std::vector<double>;

/* simple_simulator_interface::SimulationResult as built at SPCS:918 */
struct SimulationResult {
    Configuration result_config;
    Configuration target_config;
    bool did_contact = false;
    bool outcome_is_valid = true;
    uint32_t microsteps = 0;
    uint32_t resolver_iterations = 0;
    uint32_t error_flags = 0; /* FKS_PARTICLE_ERR_* */
};

/* One of the independent calls of ForwardSimulateRobotsJobs: the arguments of one
 * ForwardSimulateRobots call (target_positions holds 1 or start_positions.size()) */
struct SimulationJob {
    std::vector<Configuration> start_positions;
    std::vector<Configuration> target_positions;
    bool allow_contacts = false;
};

/* One of the independent paths of ForwardSimulateRobotsJobsAlongPaths: the arguments of one
 * ForwardSimulateRobotsAlongPath call (waypoints[leg] holds 1 or start_positions.size(), the
 * same count for every leg of the job; jobs may differ in their number of legs) */
struct SimulationPathJob {
    std::vector<Configuration> start_positions;
    std::vector<std::vector<Configuration>> waypoints;
    bool allow_contacts = false;
};

/* A policy table (fks_policy_table): the planner's execution policy as a roll-out reads it.  State
 * i stands for the configuration keys[i] and its action is to move to targets[i]; terminal[i]
 * (empty: none) marks a goal state.  A particle whose nearest state is terminal and nearer than
 * terminal_distance has arrived; one farther than max_distance from every state is lost. */
struct PolicyTable {
    std::vector<Configuration> keys;
    std::vector<Configuration> targets;
    std::vector<bool> terminal;
    double terminal_distance = 0.0;
    double max_distance = std::numeric_limits<double>::infinity();
};
/* fks_policy_select for a batch of configurations: the verdicts (an entry's index, alone or with
 * FKS_POLICY_ARRIVED, or FKS_POLICY_LOST) and the chosen entries' distances */
struct PolicySelection {
    std::vector<uint32_t> choices;
    std::vector<double> distances;
};
/* What ClusterOutcomes returns: per group the cluster number of every configuration (clusters
 * numbered in ascending order of their smallest member), the number of clusters and, when asked
 * for, the row-major n x n matrix of configuration distances (fks_cluster_configs in fks_capi.h) */
struct OutcomeClusters {
    std::vector<std::vector<uint32_t>> labels;
    std::vector<uint32_t> counts;
    std::vector<std::vector<double>> distances;
};
/* groups of configurations laid end to end for fks_cluster_configs, and the result taken apart */
struct FlatClusterGroups {
    std::vector<double> configs;
    std::vector<uint64_t> begin;
    std::vector<double> matrices;
    std::vector<uint32_t> labels, counts;
    FlatClusterGroups(const std::vector<std::vector<Configuration>>& groups, size_t W, bool want_distances) : begin(groups.size() + 1, 0) {
        size_t words = 0;
        for (size_t g = 0; g < groups.size(); ++g) {
            for (const Configuration& c : groups[g]) {
                if (c.size() != W) throw std::invalid_argument("configuration has the wrong width");
                configs.insert(configs.end(), c.begin(), c.end());
            }
            begin[g + 1] = begin[g] + groups[g].size();
            words += groups[g].size() * groups[g].size();
        }
        if (want_distances) matrices.resize(words);
        labels.resize((size_t)begin.back());
        counts.resize(groups.size());
    }
    double* matrices_or_null() { return matrices.empty() ? nullptr : matrices.data(); }
    /* (one word past the end for empty vectors: fks_cluster_configs takes NULL as "not asked for") */
    uint32_t* labels_ptr() { return labels.empty() ? &spare_ : labels.data(); }
    uint32_t* counts_ptr() { return counts.empty() ? &spare_ : counts.data(); }
    OutcomeClusters result(bool want_distances) const {
        OutcomeClusters r;
        r.counts = counts;
        size_t at = 0;
        for (size_t g = 0; g + 1 < begin.size(); ++g) {
            const size_t n = (size_t)(begin[g + 1] - begin[g]);
            r.labels.emplace_back(labels.begin() + (size_t)begin[g], labels.begin() + (size_t)begin[g + 1]);
            if (want_distances) r.distances.emplace_back(matrices.begin() + at, matrices.begin() + at + n * n);
            at += n * n;
        }
        return r;
    }

  private:
    uint32_t spare_ = 0;
};
/* What SummarizeClusters returns (fks_summarize_clusters in fks_capi.h): every array has N rows, N the
 * groups' configurations together; row group_begin[g] + c is cluster c of group g (its child state:
 * members [begin, begin + count) of `members`, their expectation and variances), the rows of empty
 * clusters are zero.  `reached` is empty when no targets were given. */
struct ClusterSummaries {
    size_t width = 0, var_width = 0; /* doubles per row of members / expectation, and of variances */
    std::vector<uint64_t> group_begin;
    std::vector<uint32_t> order, count, begin, reached;
    std::vector<double> members, expectation, variances, variance;
};
/* groups, labels and targets laid end to end for fks_summarize_clusters, with the result's arrays */
struct FlatSummaryGroups {
    std::vector<double> configs, targets;
    std::vector<uint32_t> labels;
    ClusterSummaries out;
    fks_cluster_summary summary;
    FlatSummaryGroups(const std::vector<std::vector<Configuration>>& groups, const std::vector<std::vector<uint32_t>>& group_labels,
                      const std::vector<Configuration>& group_targets, size_t W, size_t Wv) {
        if (group_labels.size() != groups.size()) throw std::invalid_argument("one label array per group");
        if (!group_targets.empty() && group_targets.size() != groups.size()) throw std::invalid_argument("one target per group, or none");
        out.width = W;
        out.var_width = Wv;
        out.group_begin.assign(groups.size() + 1, 0);
        for (size_t g = 0; g < groups.size(); ++g) {
            if (group_labels[g].size() != groups[g].size()) throw std::invalid_argument("one label per configuration");
            for (const Configuration& c : groups[g]) {
                if (c.size() != W) throw std::invalid_argument("configuration has the wrong width");
                configs.insert(configs.end(), c.begin(), c.end());
            }
            labels.insert(labels.end(), group_labels[g].begin(), group_labels[g].end());
            out.group_begin[g + 1] = out.group_begin[g] + groups[g].size();
        }
        for (const Configuration& t : group_targets) {
            if (t.size() != W) throw std::invalid_argument("target has the wrong width");
            targets.insert(targets.end(), t.begin(), t.end());
        }
        const size_t N = (size_t)out.group_begin.back();
        out.order.resize(N);
        out.count.resize(N);
        out.begin.resize(N);
        if (!group_targets.empty()) out.reached.resize(N);
        out.members.resize(N * W);
        out.expectation.resize(N * W);
        out.variances.resize(N * Wv);
        out.variance.resize(N);
        /* (a spare word for empty vectors: fks_summarize_clusters takes NULL as "not asked for") */
        summary.order = out.order.empty() ? &spare_u_ : out.order.data();
        summary.count = out.count.empty() ? &spare_u_ : out.count.data();
        summary.begin = out.begin.empty() ? &spare_u_ : out.begin.data();
        summary.reached = group_targets.empty() ? nullptr : (out.reached.empty() ? &spare_u_ : out.reached.data());
        summary.members = out.members.empty() ? &spare_d_ : out.members.data();
        summary.expectation = out.expectation.empty() ? &spare_d_ : out.expectation.data();
        summary.variances = out.variances.empty() ? &spare_d_ : out.variances.data();
        summary.variance = out.variance.empty() ? &spare_d_ : out.variance.data();
    }
    FlatSummaryGroups(const FlatSummaryGroups&) = delete; /* summary points into this object */
    FlatSummaryGroups& operator=(const FlatSummaryGroups&) = delete;
    const double* targets_or_null() const { return summary.reached ? (targets.empty() ? &spare_d_ : targets.data()) : nullptr; }
    uint64_t num_groups() const { return out.group_begin.size() - 1; }

  private:
    uint32_t spare_u_ = 0;
    double spare_d_ = 0.0;
};
/* W (linked), 3 (SE(2)), 6 (SE(3)): the doubles of a row of variances */
inline size_t SummaryVarianceWidth(const fks_robot_desc& d, size_t W) {
    return d.robot_type == FKS_ROBOT_LINKED ? W : (d.robot_type == FKS_ROBOT_SE2 ? 3 : 6);
}
/* The states SelectStates searches (fks_state_table in fks_capi.h), as flat rows: keys [S][W] (a
 * summary's expectation rows), weights [S] or empty (every weight 1), count and begin [S] or empty (a
 * summary's; begin an absolute row of members), members [rows][W] or empty. */
struct StateTable {
    std::vector<double> keys, weights, members;
    std::vector<uint32_t> count, begin;
    fks_state_table View(size_t W) const {
        if (W == 0 || keys.size() % W != 0 || members.size() % W != 0) throw std::invalid_argument("rows of the wrong width");
        const size_t S = keys.size() / W;
        if ((!weights.empty() && weights.size() != S) || (!count.empty() && count.size() != S) || (!begin.empty() && begin.size() != S))
            throw std::invalid_argument("one weight, count and begin per state");
        fks_state_table t;
        t.keys = keys.empty() ? nullptr : keys.data();
        t.weights = weights.empty() ? nullptr : weights.data();
        t.count = count.empty() ? nullptr : count.data();
        t.begin = begin.empty() ? nullptr : begin.data();
        t.members = members.empty() ? nullptr : members.data();
        t.num_states = S;
        t.num_member_rows = members.size() / W;
        return t;
    }
};
/* What SelectStates returns (fks_state_selection): choice and distance [J]; starts [J][P][W] and source
 * [J][P] when the table has count, begin and members and P > 0, empty otherwise.  draw_seed is the seed
 * the call drew with. */
struct StateSelection {
    size_t width = 0, particles = 0;
    uint64_t draw_seed = 0;
    std::vector<uint32_t> choice, source;
    std::vector<double> distance, starts;
};
/* a selection's arrays sized for J queries, and the struct that names them */
struct FlatStateSelection {
    StateSelection out;
    fks_state_selection selection;
    FlatStateSelection(const StateTable& table, size_t J, size_t P, size_t W, uint64_t draw_seed) {
        const bool drawn = P > 0 && !table.count.empty() && !table.begin.empty() && !table.members.empty();
        out.width = W;
        out.particles = drawn ? P : 0;
        out.draw_seed = draw_seed;
        out.choice.resize(J);
        out.distance.resize(J);
        if (drawn) {
            out.starts.resize(J * P * W);
            out.source.resize(J * P);
        }
        /* (a spare word for empty vectors: choice is required even for J == 0) */
        selection.choice = out.choice.empty() ? &spare_u_ : out.choice.data();
        selection.distance = out.distance.empty() ? &spare_d_ : out.distance.data();
        selection.starts = drawn ? (out.starts.empty() ? &spare_d_ : out.starts.data()) : nullptr;
        selection.source = drawn ? (out.source.empty() ? &spare_u_ : out.source.data()) : nullptr;
    }
    FlatStateSelection(const FlatStateSelection&) = delete; /* selection points into this object */
    FlatStateSelection& operator=(const FlatStateSelection&) = delete;

  private:
    uint32_t spare_u_ = 0;
    double spare_d_ = 0.0;
};
/* the draw seed of a simulator's k-th SelectStates since its generators were last reset */
inline uint64_t SelectDrawSeed(uint64_t prng_seed, uint64_t k) { return prng_seed ^ (0x9E3779B97F4A7C15ull * (k + 1)); }
/* What ForwardSimulateRobotsUnderPolicy returns: results[leg][particle] as a path's (a leg a
 * particle did not run holds the configuration it stopped at and no contact; target_config is
 * the chosen entry's action, or the configuration itself for such a leg), choices and distances
 * [leg 0 .. max_legs][particle] and legs_run[particle] (fks_forward_simulate_policy) */
struct PolicyRollout {
    std::vector<std::vector<SimulationResult>> results;
    std::vector<std::vector<uint32_t>> choices;
    std::vector<std::vector<double>> distances;
    std::vector<uint32_t> legs_run;
};
/* a PolicyTable over flat configurations of width W as the C-ABI takes it; the vectors own what
 * `table` points to */
struct FlatPolicyTable {
    std::vector<double> keys, targets;
    std::vector<uint32_t> flags;
    fks_policy_table table;
    FlatPolicyTable(const PolicyTable& policy, size_t W) {
        if (policy.keys.size() != policy.targets.size()) throw std::invalid_argument("a policy table needs one target per key");
        if (!policy.terminal.empty() && policy.terminal.size() != policy.keys.size())
            throw std::invalid_argument("a policy table's terminal flags must hold one entry per key");
        const size_t M = policy.keys.size();
        keys.resize(M * W);
        targets.resize(M * W);
        for (size_t i = 0; i < M; ++i) {
            if (policy.keys[i].size() != W || policy.targets[i].size() != W)
                throw std::invalid_argument("policy configuration has the wrong width");
            std::copy(policy.keys[i].begin(), policy.keys[i].end(), keys.begin() + i * W);
            std::copy(policy.targets[i].begin(), policy.targets[i].end(), targets.begin() + i * W);
        }
        for (size_t i = 0; i < policy.terminal.size(); ++i) flags.push_back(policy.terminal[i] ? FKS_POLICY_ENTRY_TERMINAL : 0u);
        table.keys = keys.data();
        table.targets = targets.data();
        table.flags = flags.empty() ? nullptr : flags.data();
        table.num_entries = M;
        table.terminal_distance = policy.terminal_distance;
        table.max_distance = policy.max_distance;
    }
    FlatPolicyTable(const FlatPolicyTable&) = delete;
    FlatPolicyTable& operator=(const FlatPolicyTable&) = delete;
};

/* simple_simulator_interface::ForwardSimulationStepTrace as filled at SPCS:1583-1595,
 * 1615-1618, 1701-1704, 1712-1715, 1776-1779.  `kinds` tags each configuration
 * with the FKS_TRACE_* push site it came from. */
struct ForwardSimulationContactResolverStepTrace {
    std::vector<Configuration> contact_resolution_steps;
    std::vector<uint32_t> kinds;
};
struct ForwardSimulationResolverTrace {
    std::vector<double> control_input;      /* real_control_input = u * dt (SPCS:1549) */
    std::vector<double> control_input_step; /* real_control_input / microsteps (SPCS:1568) */
    std::vector<ForwardSimulationContactResolverStepTrace> contact_resolver_steps;
};
struct ForwardSimulationStepTrace {
    std::vector<ForwardSimulationResolverTrace> resolver_steps;
    bool truncated = false; /* records beyond the trace capacity were dropped */
};

/* visualization_msgs::Marker reduced to plain data (ROS is not part of this
 * repository): what the reference's display helpers fill in */
struct Marker {
    std::string ns;
    int32_t id = 0;
    std::string type; /* "SPHERE_LIST", "LINE_LIST" */
    std::string frame_id;
    std::array<double, 3> scale{{0.0, 0.0, 0.0}};
    std::array<float, 4> color{{0.0f, 0.0f, 0.0f, 1.0f}};
    std::vector<std::array<double, 3>> points;
    std::vector<std::array<float, 4>> colors;
};

/* fast_kinematic_simulator::GetDefaultSolverParameters (FKS.hpp:13-16) */
inline fks_solver_params GetDefaultSolverParameters() {
    fks_solver_params p;
    check(fks_default_solver_params(&p), nullptr, "GetDefaultSolverParameters");
    return p;
}

/* A flattened robot (fks_robot_desc) that owns its arrays: the immutable_robot
 * argument of ForwardSimulateRobots (SPCS:788).  Build it once per robot. */
class RobotDescription {
  public:
    fks_robot_type type = FKS_ROBOT_LINKED;
    int32_t num_links = 1;
    int32_t num_dofs = 0;
    double base_transform[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<fks_joint_desc> joints;
    std::vector<int32_t> geometry_link;
    std::vector<uint32_t> geometry_point_offset{0};
    std::vector<double> points; /* x, y, z, w per point */
    std::vector<int32_t> allowed_pairs; /* geometry index pairs */
    std::vector<fks_dof_controller> controllers;
    std::vector<double> distance_weights;
    /* empty, or one per dof: SampledUncertainVelocityActuator bins (num_bins 0 = truncated
     * normal); the bound/sample arrays they point to must outlive the simulator calls */
    std::vector<fks_sampled_actuator> sampled_actuators;

    /* geometry `g` of link `link`: points as (x, y, z, w) quadruples */
    int32_t AddGeometry(int32_t link, const std::vector<double>& xyzw) {
        if (xyzw.size() % 4 != 0) throw std::invalid_argument("points are x, y, z, w quadruples");
        geometry_link.push_back(link);
        points.insert(points.end(), xyzw.begin(), xyzw.end());
        geometry_point_offset.push_back((uint32_t)(points.size() / 4));
        return (int32_t)geometry_link.size() - 1;
    }
    void AllowSelfCollision(int32_t geometry_a, int32_t geometry_b) {
        allowed_pairs.push_back(geometry_a);
        allowed_pairs.push_back(geometry_b);
    }
    /* dof `dof` draws its actuation noise from `bins` (SampledUncertainVelocityActuator,
     * UNC:224-281; simple_uncertainty_models::SetSampledActuator builds them from a LoadModel
     * result); `owner` keeps the arrays the bins point to alive with this description */
    void SetSampledActuator(int32_t dof, const fks_sampled_actuator& bins, std::shared_ptr<const void> owner) {
        if (dof < 0 || dof >= NumDofs()) throw std::invalid_argument("SetSampledActuator: dof out of range");
        if (sampled_actuators.size() != (size_t)NumDofs()) sampled_actuators.assign((size_t)NumDofs(), fks_sampled_actuator{});
        sampled_actuators[(size_t)dof] = bins;
        sampled_owners_.push_back(std::move(owner));
    }
    int32_t NumDofs() const { return type == FKS_ROBOT_SE2 ? 3 : (type == FKS_ROBOT_SE3 ? 6 : num_dofs); }
    int32_t ConfigurationWidth() const {
        return type == FKS_ROBOT_SE2 ? 3 : (type == FKS_ROBOT_SE3 ? 12 : num_dofs);
    }
    /* every byte the simulator receives (fields, tables and the sampled-actuator bins the
     * pointers reach): equal fingerprints mean the same robot for the GPU */
    std::vector<unsigned char> Fingerprint() const {
        std::vector<unsigned char> out;
        auto put = [&out](const void* p, size_t n) {
            const unsigned char* b = static_cast<const unsigned char*>(p);
            out.insert(out.end(), b, b + n);
        };
        auto put_size = [&put](size_t n) {
            const uint64_t v = (uint64_t)n;
            put(&v, sizeof(v));
        };
        put(&type, sizeof(type));
        put(&num_links, sizeof(num_links));
        put(&num_dofs, sizeof(num_dofs));
        put(base_transform, sizeof(base_transform));
        put_size(joints.size());
        put(joints.data(), joints.size() * sizeof(fks_joint_desc));
        put_size(geometry_link.size());
        put(geometry_link.data(), geometry_link.size() * sizeof(int32_t));
        put_size(geometry_point_offset.size());
        put(geometry_point_offset.data(), geometry_point_offset.size() * sizeof(uint32_t));
        put_size(points.size());
        put(points.data(), points.size() * sizeof(double));
        put_size(allowed_pairs.size());
        put(allowed_pairs.data(), allowed_pairs.size() * sizeof(int32_t));
        put_size(controllers.size());
        put(controllers.data(), controllers.size() * sizeof(fks_dof_controller));
        put_size(distance_weights.size());
        put(distance_weights.data(), distance_weights.size() * sizeof(double));
        put_size(sampled_actuators.size());
        for (const fks_sampled_actuator& a : sampled_actuators) {
            put(&a.num_bins, sizeof(a.num_bins));
            put(&a.bin_elements, sizeof(a.bin_elements));
            if (a.num_bins && a.bin_bounds) put(a.bin_bounds, 2 * (size_t)a.num_bins * sizeof(double));
            if (a.num_bins && a.bin_samples) put(a.bin_samples, (size_t)a.num_bins * a.bin_elements * sizeof(double));
        }
        return out;
    }
  private:
    std::vector<std::shared_ptr<const void>> sampled_owners_;

  public:
    fks_robot_desc View() const {
        fks_robot_desc d{};
        d.robot_type = type;
        d.num_links = num_links;
        d.num_joints = (int32_t)joints.size();
        d.num_geometries = (int32_t)geometry_link.size();
        d.num_dofs = num_dofs;
        d.num_allowed_pairs = (int32_t)(allowed_pairs.size() / 2);
        for (int i = 0; i < 12; ++i) d.base_transform[i] = base_transform[i];
        d.joints = joints.empty() ? nullptr : joints.data();
        d.geometry_link = geometry_link.data();
        d.geometry_point_offset = geometry_point_offset.data();
        d.points = points.data();
        d.allowed_pairs = allowed_pairs.empty() ? nullptr : allowed_pairs.data();
        d.controllers = controllers.data();
        d.distance_weights = distance_weights.empty() ? nullptr : distance_weights.data();
        d.sampled_actuators = sampled_actuators.empty() ? nullptr : sampled_actuators.data();
        return d;
    }
};

/* SimpleParticleContactSimulator on one or several MI355X devices (DeviceSet: a batch is
 * sharded by particle id over as many devices as keep at least ShardThreshold() particles
 * each, bit-identical to one device).  The stacked-Jacobian resolver is always used, as the reference factories
 * hard-wire (FKS.cpp:22,45,68). */
class HipParticleContactSimulator {
  public:
    using DisplayFn = std::function<void(const void*)>;

    HipParticleContactSimulator(const fks_environment& environment, const fks_solver_params& solver_config,
                                double simulation_controller_frequency, uint64_t prng_seed, int32_t debug_level,
                                const std::vector<int32_t>& devices)
        : dev_(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level, devices) {
        ctx_ = dev_.primary();
        select_seed_ = prng_seed;
        forward_steps_ = (uint32_t)std::max(1.0, solver_config.forward_simulation_time * simulation_controller_frequency);
        resolution_ = environment.collision_map.resolution;
        /* ResetGenerators (SPCS:457-471): the first per-thread generator */
        std::mt19937_64 prng(prng_seed);
        std::uniform_int_distribution<uint64_t> seed_dist(0, std::numeric_limits<uint64_t>::max());
        rng_ = std::mt19937_64(seed_dist(prng));
    }
    HipParticleContactSimulator(const fks_environment& environment, const fks_solver_params& solver_config,
                                double simulation_controller_frequency, uint64_t prng_seed, int32_t debug_level,
                                int32_t device = 0)
        : HipParticleContactSimulator(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level,
                                      std::vector<int32_t>{device}) {}

    const std::vector<int32_t>& Devices() const { return dev_.devices(); }
    void SetShardThreshold(uint64_t particles_per_device) { dev_.set_shard_threshold(particles_per_device); }
    uint64_t ShardThreshold() const { return dev_.shard_threshold(); }
    bool LastBatchSharded() const { return dev_.last_sharded(); }
    int32_t LastBatchDevices() const { return dev_.last_devices(); }
    /* build `robot`'s shape-specialised kernel on every device now (see
     * fast_kinematic_simulator.hpp PrepareKernels); never throws on a failed build.  batched:
     * also the module of path, job and path-job batches (BatchedSpecializationStatus) */
    fks::SpecializationStatus PrepareKernels(const RobotDescription& robot, bool batched = false) {
        SetRobot(robot);
        return dev_.prepare_kernels(FKS_SPECIALIZE_ON, batched);
    }
    fks::SpecializationStatus SpecializationStatus() const { return dev_.specialization_status(); }
    fks::SpecializationStatus BatchedSpecializationStatus() const { return dev_.batched_specialization_status(); }

    /* GetFrame (SPCS:517-520) */
    std::string GetFrame() const { return frame_; }
    void SetFrame(const std::string& frame) { frame_ = frame; }
    /* GetRandomGenerator (SPCS:473-481), for the caller's own sampling; the simulation's
     * noise is the counter RNG keyed by (seed, call, particle, step, microstep, dof) */
    std::mt19937_64& GetRandomGenerator() { return rng_; }

    /* fks_kinematics over a batch: FKS_KIN_LINK_TRANSFORMS -> links x 12 per config,
     * FKS_KIN_POINTS -> points x 3, FKS_KIN_APPLY_CONTROL_INPUT -> config width */
    std::vector<double> Kinematics(const RobotDescription& robot, int32_t mode, const std::vector<Configuration>& configs,
                                   const std::vector<std::vector<double>>& inputs = {}) {
        SetRobot(robot);
        int32_t links = 0, points = 0, dofs = 0, width = 0;
        check(fks_robot_sizes(ctx_, &links, &points, &dofs, &width), ctx_, "fks_robot_sizes");
        const size_t n = configs.size(), W = (size_t)width;
        std::vector<double> c(n * W), u;
        for (size_t i = 0; i < n; ++i) {
            if (configs[i].size() != W) throw std::invalid_argument("configuration has the wrong width");
            std::copy(configs[i].begin(), configs[i].end(), c.begin() + i * W);
        }
        if (mode == FKS_KIN_APPLY_CONTROL_INPUT) {
            if (inputs.size() != n) throw std::invalid_argument("one control input per configuration");
            for (const auto& in : inputs) {
                if (in.size() != (size_t)dofs) throw std::invalid_argument("control input has the wrong width");
                u.insert(u.end(), in.begin(), in.end());
            }
        }
        const size_t per = mode == FKS_KIN_LINK_TRANSFORMS ? 12u * (size_t)links : (mode == FKS_KIN_POINTS ? 3u * (size_t)points : W);
        std::vector<double> out(n * per);
        check(fks_kinematics(ctx_, mode, c.data(), n, u.empty() ? nullptr : u.data(), out.data()), ctx_,
              "fks_kinematics");
        return out;
    }

    /* Get3dPointForConfig (SPCS:776-786): origin of the last geometry's link, w = 1 */
    std::array<double, 4> Get3dPointForConfig(const RobotDescription& immutable_robot, const Configuration& config) {
        const std::vector<double> T = Kinematics(immutable_robot, FKS_KIN_LINK_TRANSFORMS, {config});
        const size_t l = (size_t)immutable_robot.geometry_link.back();
        return {{T[12 * l + 3], T[12 * l + 7], T[12 * l + 11], 1.0}};
    }

    /* MakeConfigurationDisplayRep for POINTS geometries (SPCS:634-688) */
    std::vector<Marker> MakeConfigurationDisplayRep(const RobotDescription& immutable_robot, const Configuration& configuration,
                                                    const std::array<float, 4>& color, int32_t starting_index,
                                                    const std::string& config_marker_ns) {
        const std::vector<double> pts = Kinematics(immutable_robot, FKS_KIN_POINTS, {configuration});
        Marker m;
        m.ns = config_marker_ns;
        m.id = starting_index;
        m.type = "SPHERE_LIST";
        m.frame_id = frame_;
        m.scale = {{resolution_, resolution_, resolution_}};
        m.color = color;
        for (size_t i = 0; i < pts.size() / 3; ++i) {
            m.points.push_back({{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}});
            const double* p = immutable_robot.points.data() + 4 * i;
            const bool zero = (p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]) == 0.0;
            m.colors.push_back(zero ? std::array<float, 4>{{0.0f, 0.0f, 0.0f, 1.0f}} : color);
        }
        return {m};
    }

    /* MakeControlInputDisplayRep (SPCS:719-774): each point before and after the clean input */
    std::vector<Marker> MakeControlInputDisplayRep(const RobotDescription& immutable_robot, const Configuration& configuration,
                                                   const std::vector<double>& control_input, const std::array<float, 4>& color,
                                                   int32_t starting_index, const std::string& control_input_marker_ns) {
        const std::vector<double> after = Kinematics(immutable_robot, FKS_KIN_APPLY_CONTROL_INPUT, {configuration}, {control_input});
        const std::vector<double> pts =
            Kinematics(immutable_robot, FKS_KIN_POINTS, {configuration, Configuration(after.begin(), after.end())});
        const size_t P = pts.size() / 6;
        Marker m;
        m.ns = control_input_marker_ns;
        m.id = starting_index;
        m.type = "LINE_LIST";
        m.frame_id = frame_;
        m.scale = {{resolution_ * 0.5, resolution_ * 0.5, resolution_ * 0.5}};
        m.color = color;
        for (size_t i = 0; i < P; ++i) {
            m.points.push_back({{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}});
            m.points.push_back({{pts[3 * (P + i)], pts[3 * (P + i) + 1], pts[3 * (P + i) + 2]}});
            m.colors.push_back(color);
            m.colors.push_back(color);
        }
        return {m};
    }

    /* SPCS:446-455 */
    int32_t GetDebugLevel() const { return fks_get_debug_level(ctx_); }
    int32_t SetDebugLevel(int32_t debug_level) { return dev_.set_debug_level(debug_level); }

    /* SPCS:488-512: the eight resolve counters, by the reference's names */
    std::vector<std::pair<std::string, double>> GetStatistics() const {
        const fks_statistics s = dev_.statistics();
        return {{"successful_resolves", (double)s.successful_resolves},
                {"unsuccessful_resolves", (double)s.unsuccessful_resolves},
                {"free_resolves", (double)s.free_resolves},
                {"collision_resolves", (double)s.collision_resolves},
                {"fallback_resolves", (double)s.fallback_resolves},
                {"unsuccessful_env_collision_resolves", (double)s.unsuccessful_env_collision_resolves},
                {"unsuccessful_self_collision_resolves", (double)s.unsuccessful_self_collision_resolves},
                {"recovered_unsuccessful_resolves", (double)s.recovered_unsuccessful_resolves}};
    }
    void ResetStatistics() { dev_.reset_statistics(); }
    /* SPCS:457-471 */
    void ResetGenerators(uint64_t prng_seed) {
        dev_.reset_generators(prng_seed);
        select_seed_ = prng_seed;
        select_calls_ = 0;
    }

    /* ForwardSimulateRobots (SPCS:788-804).  display_fn is accepted for interface
     * parity; the batch path never draws (SPCS:801 passes enable_tracing=false). */
    std::vector<SimulationResult> ForwardSimulateRobots(const RobotDescription& immutable_robot,
                                                        const std::vector<Configuration>& start_positions,
                                                        const std::vector<Configuration>& target_positions,
                                                        bool allow_contacts, const DisplayFn& display_fn = {}) {
        (void)display_fn;
        return Simulate(immutable_robot, start_positions, target_positions, allow_contacts, false);
    }
    /* The batch along a waypoint path in one launch (fks_forward_simulate_path; no reference
     * counterpart: the planner's edge-after-edge loop over ForwardSimulateRobots).  waypoints[k]
     * holds 1 or start_positions.size() configurations, the same count for every leg.
     * results[k][i] is what the k-th of waypoints.size() chained ForwardSimulateRobots calls
     * returns for particle i, each starting from the result_configs of the one before, bit for
     * bit; a particle starts its next leg when its own leg ends. */
    std::vector<std::vector<SimulationResult>> ForwardSimulateRobotsAlongPath(const RobotDescription& immutable_robot,
                                                                              const std::vector<Configuration>& start_positions,
                                                                              const std::vector<std::vector<Configuration>>& waypoints,
                                                                              bool allow_contacts) {
        if (waypoints.empty()) throw std::invalid_argument("a path needs at least one leg");
        const size_t K = waypoints.size(), n = start_positions.size(), nt = waypoints[0].size();
        if (n > 0 && nt != 1 && nt != n) throw std::invalid_argument("every leg must hold 1 or start_positions.size() waypoints");
        SetRobot(immutable_robot);
        const size_t W = (size_t)immutable_robot.ConfigurationWidth();
        std::vector<double> s(n * W), t(K * nt * W), out(K * n * W);
        for (size_t i = 0; i < n; ++i) {
            if (start_positions[i].size() != W) throw std::invalid_argument("start configuration has the wrong width");
            std::copy(start_positions[i].begin(), start_positions[i].end(), s.begin() + i * W);
        }
        for (size_t k = 0; k < K; ++k) {
            if (waypoints[k].size() != nt) throw std::invalid_argument("every leg must hold the same number of waypoints");
            for (size_t i = 0; i < nt; ++i) {
                if (waypoints[k][i].size() != W) throw std::invalid_argument("waypoint configuration has the wrong width");
                std::copy(waypoints[k][i].begin(), waypoints[k][i].end(), t.begin() + (k * nt + i) * W);
            }
        }
        std::vector<uint8_t> collided(K * n);
        std::vector<uint32_t> micro(K * n), resolver(K * n), errors(K * n);
        dev_.simulate_path(s.data(), n, t.data(), K, nt, allow_contacts, out.data(), collided.data(), micro.data(), resolver.data(),
                           errors.data(), "ForwardSimulateRobotsAlongPath");
        std::vector<std::vector<SimulationResult>> results(K, std::vector<SimulationResult>(n));
        for (size_t k = 0; k < K; ++k)
            for (size_t i = 0; i < n; ++i) {
                SimulationResult& r = results[k][i];
                const size_t row = k * n + i;
                r.result_config.assign(out.begin() + row * W, out.begin() + (row + 1) * W);
                r.target_config = nt == n ? waypoints[k][i] : waypoints[k][0];
                r.did_contact = collided[row] != 0;
                r.outcome_is_valid = true;
                r.microsteps = micro[row];
                r.resolver_iterations = resolver[row];
                r.error_flags = errors[row];
            }
        return results;
    }
    /* The batch rolled out under a policy table in one launch (fks_forward_simulate_policy; the
     * planner's SimulateExectionPolicy loop: after every ForwardSimulateRobot the policy looks at
     * where the particle ended, picks the nearest state, and that state's action is the next
     * target).  Before each of at most max_legs legs every particle selects its entry
     * (PolicySelect); a lost or arrived particle stops.  Bit for bit what that sequence of plain
     * calls returns; a particle starts its next leg when its own leg ends. */
    PolicyRollout ForwardSimulateRobotsUnderPolicy(const RobotDescription& immutable_robot,
                                                   const std::vector<Configuration>& start_positions, const PolicyTable& policy,
                                                   size_t max_legs, bool allow_contacts) {
        if (max_legs == 0) throw std::invalid_argument("a roll-out needs at least one leg");
        SetRobot(immutable_robot);
        const size_t W = (size_t)immutable_robot.ConfigurationWidth(), K = max_legs, n = start_positions.size();
        const FlatPolicyTable flat(policy, W);
        std::vector<double> s(n * W), out(K * n * W), dist((K + 1) * n);
        for (size_t i = 0; i < n; ++i) {
            if (start_positions[i].size() != W) throw std::invalid_argument("start configuration has the wrong width");
            std::copy(start_positions[i].begin(), start_positions[i].end(), s.begin() + i * W);
        }
        std::vector<uint8_t> collided(K * n);
        std::vector<uint32_t> micro(K * n), resolver(K * n), errors(K * n), choice((K + 1) * n), legs(n);
        dev_.simulate_policy(s.data(), n, flat.table, K, allow_contacts, out.data(), collided.data(), micro.data(), resolver.data(),
                             errors.data(), choice.data(), dist.data(), legs.data(), "ForwardSimulateRobotsUnderPolicy");
        PolicyRollout r;
        r.results.assign(K, std::vector<SimulationResult>(n));
        r.choices.assign(K + 1, std::vector<uint32_t>(n));
        r.distances.assign(K + 1, std::vector<double>(n));
        r.legs_run = legs;
        for (size_t k = 0; k <= K; ++k)
            for (size_t i = 0; i < n; ++i) {
                r.choices[k][i] = choice[k * n + i];
                r.distances[k][i] = dist[k * n + i];
            }
        for (size_t k = 0; k < K; ++k)
            for (size_t i = 0; i < n; ++i) {
                SimulationResult& res = r.results[k][i];
                const size_t row = k * n + i;
                res.result_config.assign(out.begin() + row * W, out.begin() + (row + 1) * W);
                res.target_config = k < legs[i] ? policy.targets[choice[row] & ~FKS_POLICY_ARRIVED] : res.result_config;
                res.did_contact = collided[row] != 0;
                res.outcome_is_valid = true;
                res.microsteps = micro[row];
                res.resolver_iterations = resolver[row];
                res.error_flags = errors[row];
            }
        return r;
    }
    /* fks_policy_select: the selection of a policy table for a batch of configurations on the
     * host, with the kernels' arithmetic and without a simulator (the planner's single query
     * during real execution, QueryBestAction) */
    static PolicySelection PolicySelect(const RobotDescription& robot, const PolicyTable& policy,
                                        const std::vector<Configuration>& configs) {
        const size_t W = (size_t)robot.ConfigurationWidth(), n = configs.size();
        const FlatPolicyTable flat(policy, W);
        std::vector<double> q(n * W);
        for (size_t i = 0; i < n; ++i) {
            if (configs[i].size() != W) throw std::invalid_argument("configuration has the wrong width");
            std::copy(configs[i].begin(), configs[i].end(), q.begin() + i * W);
        }
        PolicySelection sel;
        sel.choices.resize(n);
        sel.distances.resize(n);
        const fks_robot_desc d = robot.View();
        const fks_status st = fks_policy_select(&d, &flat.table, q.data(), n, sel.choices.data(), sel.distances.data());
        if (st != FKS_OK) throw SimulatorError(st, std::string("PolicySelect: ") + fks_status_string(st));
        return sel;
    }
    /* The planner's step after every forward batch (fks_cluster_configs_ctx): each group's
     * outcomes (one group per job) clustered by the robot's configuration distance, complete link
     * under `threshold`, in one launch.  Byte for byte what ClusterOutcomesHost returns; no call
     * index is consumed and no statistics move. */
    OutcomeClusters ClusterOutcomes(const RobotDescription& immutable_robot, const std::vector<std::vector<Configuration>>& groups,
                                    double threshold, bool want_distances = false) {
        SetRobot(immutable_robot);
        FlatClusterGroups flat(groups, (size_t)immutable_robot.ConfigurationWidth(), want_distances);
        dev_.cluster_configs(flat.configs.data(), flat.begin.data(), groups.size(), threshold, flat.matrices_or_null(), flat.labels_ptr(),
                             flat.counts_ptr(), "ClusterOutcomes");
        return flat.result(want_distances);
    }
    /* fks_cluster_configs: the same on the host, with the kernels' arithmetic and without a simulator */
    static OutcomeClusters ClusterOutcomesHost(const RobotDescription& robot, const std::vector<std::vector<Configuration>>& groups,
                                               double threshold, bool want_distances = false) {
        FlatClusterGroups flat(groups, (size_t)robot.ConfigurationWidth(), want_distances);
        const fks_robot_desc d = robot.View();
        const fks_status st = fks_cluster_configs(&d, flat.configs.data(), flat.begin.data(), groups.size(), threshold,
                                                  flat.matrices_or_null(), flat.labels_ptr(), flat.counts_ptr());
        if (st != FKS_OK) throw SimulatorError(st, std::string("ClusterOutcomesHost: ") + fks_status_string(st));
        return flat.result(want_distances);
    }
    /* The planner's step after the clustering (fks_summarize_clusters_ctx): every cluster of every
     * group made into a child state (its regrouped members, their expectation, per-dimension and
     * scalar variances and, with one target per group, the members within reached_distance of it),
     * in one launch.  labels[g] is what ClusterOutcomes returned for groups[g].  Byte for byte what
     * SummarizeClustersHost returns; no call index is consumed and no statistics move. */
    ClusterSummaries SummarizeClusters(const RobotDescription& immutable_robot, const std::vector<std::vector<Configuration>>& groups,
                                       const std::vector<std::vector<uint32_t>>& labels, const std::vector<Configuration>& targets = {},
                                       double reached_distance = 0.0) {
        SetRobot(immutable_robot);
        const size_t W = (size_t)immutable_robot.ConfigurationWidth();
        FlatSummaryGroups flat(groups, labels, targets, W, SummaryVarianceWidth(immutable_robot.View(), W));
        dev_.summarize_clusters(flat.configs.data(), flat.out.group_begin.data(), flat.num_groups(), flat.labels.data(),
                                flat.targets_or_null(), reached_distance, &flat.summary, "SummarizeClusters");
        return std::move(flat.out);
    }
    /* fks_summarize_clusters: the same on the host, with the kernels' arithmetic and without a simulator */
    static ClusterSummaries SummarizeClustersHost(const RobotDescription& robot, const std::vector<std::vector<Configuration>>& groups,
                                                  const std::vector<std::vector<uint32_t>>& labels,
                                                  const std::vector<Configuration>& targets = {}, double reached_distance = 0.0) {
        const size_t W = (size_t)robot.ConfigurationWidth();
        const fks_robot_desc d = robot.View();
        FlatSummaryGroups flat(groups, labels, targets, W, SummaryVarianceWidth(d, W));
        const fks_status st = fks_summarize_clusters(&d, flat.configs.data(), flat.out.group_begin.data(), flat.num_groups(),
                                                     flat.labels.data(), flat.targets_or_null(), reached_distance, &flat.summary);
        if (st != FKS_OK) throw SimulatorError(st, std::string("SummarizeClustersHost: ") + fks_status_string(st));
        return std::move(flat.out);
    }
    /* The planner's step between a summary and the next jobs (fks_select_states_ctx): for every query the
     * nearest state of `table` under its weights, and the chosen state's members drawn into P starts, in
     * two launches.  queries are flat configurations.  The draw seed is SelectDrawSeed(prng_seed, k) for
     * the k-th selection since the generators were last reset (StateSelection.draw_seed names it); no
     * call index is consumed and no statistics move.  Byte for byte what SelectStatesHost returns for the
     * same seed. */
    StateSelection SelectStates(const RobotDescription& immutable_robot, const StateTable& table, const std::vector<Configuration>& queries,
                                uint32_t num_particles = 0) {
        SetRobot(immutable_robot);
        const size_t W = (size_t)immutable_robot.ConfigurationWidth();
        const std::vector<double> flat = FlatQueries(queries, W);
        FlatStateSelection sel(table, queries.size(), num_particles, W, SelectDrawSeed(select_seed_, select_calls_++));
        dev_.select_states(table.View(W), flat.data(), queries.size(), num_particles, sel.out.draw_seed, sel.selection, "SelectStates");
        return std::move(sel.out);
    }
    /* the same on device buffers (fks_select_states_device): every pointer of d_table and d_out and d_queries
     * are in HBM, d_out.starts fit to be the next jobs' starts; returns the draw seed used */
    uint64_t SelectStates(const RobotDescription& immutable_robot, const fks_state_table& d_table, const double* d_queries,
                          uint64_t num_queries, uint32_t num_particles, const fks_state_selection& d_out, void* stream = nullptr,
                          bool synchronize = true) {
        SetRobot(immutable_robot);
        const uint64_t seed = SelectDrawSeed(select_seed_, select_calls_++);
        dev_.select_states_device(d_table, d_queries, num_queries, num_particles, seed, d_out, stream, synchronize, "SelectStates");
        return seed;
    }
    /* fks_select_states: the same on the host, with the kernels' arithmetic and without a simulator */
    static StateSelection SelectStatesHost(const RobotDescription& robot, const StateTable& table, const std::vector<Configuration>& queries,
                                           uint32_t num_particles, uint64_t draw_seed) {
        const size_t W = (size_t)robot.ConfigurationWidth();
        const fks_robot_desc d = robot.View();
        const std::vector<double> flat = FlatQueries(queries, W);
        FlatStateSelection sel(table, queries.size(), num_particles, W, draw_seed);
        const fks_state_table t = table.View(W);
        const fks_status st = fks_select_states(&d, &t, flat.data(), queries.size(), num_particles, draw_seed, &sel.selection);
        if (st != FKS_OK) throw SimulatorError(st, std::string("SelectStatesHost: ") + fks_status_string(st));
        return std::move(sel.out);
    }
    static std::vector<double> FlatQueries(const std::vector<Configuration>& queries, size_t W) {
        std::vector<double> flat;
        for (const Configuration& q : queries) {
            if (q.size() != W) throw std::invalid_argument("query has the wrong width");
            flat.insert(flat.end(), q.begin(), q.end());
        }
        if (flat.empty()) flat.push_back(0.0); /* a pointer for J == 0 */
        return flat;
    }
    /* Many independent calls in one launch (fks_forward_simulate_jobs; no reference counterpart:
     * the planner's stream of small ForwardSimulateRobots / ReverseSimulateRobots calls, whose
     * semantics are the same, SPCS:838-841).  results[j] is what the j-th of jobs.size() plain
     * calls issued one after the other returns, bit for bit; the jobs' particles share the
     * device side by side. */
    std::vector<std::vector<SimulationResult>> ForwardSimulateRobotsJobs(const RobotDescription& immutable_robot,
                                                                         const std::vector<SimulationJob>& jobs) {
        if (jobs.empty()) throw std::invalid_argument("a job batch needs at least one job");
        SetRobot(immutable_robot);
        const size_t W = (size_t)immutable_robot.ConfigurationWidth(), J = jobs.size();
        size_t N = 0, NT = 0;
        for (const SimulationJob& job : jobs) {
            const size_t n = job.start_positions.size(), nt = job.target_positions.size();
            if (n > 0 && nt != 1 && nt != n) throw std::invalid_argument("a job must hold 1 or start_positions.size() targets");
            N += n;
            NT += n > 0 ? nt : 0;
        }
        std::vector<double> s(N * W), t(NT * W), out(N * W);
        std::vector<uint8_t> collided(N);
        std::vector<uint32_t> micro(N), resolver(N), errors(N);
        std::vector<fks_job> cj(J);
        size_t at = 0, tat = 0;
        for (size_t j = 0; j < J; ++j) {
            const SimulationJob& job = jobs[j];
            const size_t n = job.start_positions.size(), nt = n > 0 ? job.target_positions.size() : 0;
            for (size_t i = 0; i < n; ++i) {
                if (job.start_positions[i].size() != W) throw std::invalid_argument("start configuration has the wrong width");
                std::copy(job.start_positions[i].begin(), job.start_positions[i].end(), s.begin() + (at + i) * W);
            }
            for (size_t i = 0; i < nt; ++i) {
                if (job.target_positions[i].size() != W) throw std::invalid_argument("target configuration has the wrong width");
                std::copy(job.target_positions[i].begin(), job.target_positions[i].end(), t.begin() + (tat + i) * W);
            }
            fks_job& c = cj[j];
            c = fks_job();
            c.starts = s.data() + at * W;
            c.n = n;
            c.targets = t.data() + tat * W;
            c.num_targets = n > 0 ? nt : 1;
            c.allow_contacts = job.allow_contacts ? 1 : 0;
            c.out_positions = out.data() + at * W;
            c.out_collided = collided.data() + at;
            c.out_microsteps = micro.data() + at;
            c.out_resolver_iterations = resolver.data() + at;
            c.out_error_flags = errors.data() + at;
            at += n;
            tat += nt;
        }
        dev_.simulate_jobs(cj.data(), J, "ForwardSimulateRobotsJobs");
        std::vector<std::vector<SimulationResult>> results(J);
        size_t row = 0;
        for (size_t j = 0; j < J; ++j) {
            const SimulationJob& job = jobs[j];
            const size_t n = job.start_positions.size();
            results[j].resize(n);
            for (size_t i = 0; i < n; ++i, ++row) {
                SimulationResult& r = results[j][i];
                r.result_config.assign(out.begin() + row * W, out.begin() + (row + 1) * W);
                r.target_config = job.target_positions.size() == n ? job.target_positions[i] : job.target_positions[0];
                r.did_contact = collided[row] != 0;
                r.outcome_is_valid = true;
                r.microsteps = micro[row];
                r.resolver_iterations = resolver[row];
                r.error_flags = errors[row];
            }
        }
        return results;
    }
    /* Many independent waypoint paths in one launch (fks_forward_simulate_path_jobs; no reference
     * counterpart: a planner iteration's edges, each simulated forward to its target and back,
     * ForwardSimulateRobots then ReverseSimulateRobots, SPCS:788-822).  results[j][k][i] is what
     * the j-th of jobs.size() ForwardSimulateRobotsAlongPath calls issued one after the other
     * returns for leg k and particle i, bit for bit; the jobs may differ in their number of legs. */
    std::vector<std::vector<std::vector<SimulationResult>>> ForwardSimulateRobotsJobsAlongPaths(
        const RobotDescription& immutable_robot, const std::vector<SimulationPathJob>& jobs) {
        if (jobs.empty()) throw std::invalid_argument("a job batch needs at least one job");
        SetRobot(immutable_robot);
        const size_t W = (size_t)immutable_robot.ConfigurationWidth(), J = jobs.size();
        size_t N = 0, NT = 0, R = 0;
        for (const SimulationPathJob& job : jobs) {
            if (job.waypoints.empty()) throw std::invalid_argument("a path needs at least one leg");
            const size_t n = job.start_positions.size(), nt = job.waypoints[0].size(), K = job.waypoints.size();
            if (n > 0 && nt != 1 && nt != n) throw std::invalid_argument("every leg must hold 1 or start_positions.size() waypoints");
            for (const auto& leg : job.waypoints)
                if (leg.size() != nt) throw std::invalid_argument("every leg must hold the same number of waypoints");
            N += n;
            NT += n > 0 ? nt * K : 0;
            R += n * K;
        }
        std::vector<double> s(N * W), t(NT * W), out(R * W);
        std::vector<uint8_t> collided(R);
        std::vector<uint32_t> micro(R), resolver(R), errors(R);
        std::vector<fks_path_job> cj(J);
        size_t at = 0, tat = 0, oat = 0;
        for (size_t j = 0; j < J; ++j) {
            const SimulationPathJob& job = jobs[j];
            const size_t n = job.start_positions.size(), K = job.waypoints.size(), nt = n > 0 ? job.waypoints[0].size() : 0;
            for (size_t i = 0; i < n; ++i) {
                if (job.start_positions[i].size() != W) throw std::invalid_argument("start configuration has the wrong width");
                std::copy(job.start_positions[i].begin(), job.start_positions[i].end(), s.begin() + (at + i) * W);
            }
            for (size_t k = 0; k < K; ++k)
                for (size_t i = 0; i < nt; ++i) {
                    if (job.waypoints[k][i].size() != W) throw std::invalid_argument("waypoint configuration has the wrong width");
                    std::copy(job.waypoints[k][i].begin(), job.waypoints[k][i].end(), t.begin() + (tat + k * nt + i) * W);
                }
            fks_path_job& c = cj[j];
            c = fks_path_job();
            c.starts = s.data() + at * W;
            c.n = n;
            c.waypoints = t.data() + tat * W;
            c.num_legs = K;
            c.num_targets = n > 0 ? nt : 1;
            c.allow_contacts = job.allow_contacts ? 1 : 0;
            c.out_positions = out.data() + oat * W;
            c.out_collided = collided.data() + oat;
            c.out_microsteps = micro.data() + oat;
            c.out_resolver_iterations = resolver.data() + oat;
            c.out_error_flags = errors.data() + oat;
            at += n;
            tat += nt * K;
            oat += n * K;
        }
        dev_.simulate_path_jobs(cj.data(), J, "ForwardSimulateRobotsJobsAlongPaths");
        std::vector<std::vector<std::vector<SimulationResult>>> results(J);
        size_t row = 0;
        for (size_t j = 0; j < J; ++j) {
            const SimulationPathJob& job = jobs[j];
            const size_t n = job.start_positions.size(), K = job.waypoints.size();
            results[j].assign(K, std::vector<SimulationResult>(n));
            for (size_t k = 0; k < K; ++k)
                for (size_t i = 0; i < n; ++i, ++row) {
                    SimulationResult& r = results[j][k][i];
                    r.result_config.assign(out.begin() + row * W, out.begin() + (row + 1) * W);
                    r.target_config = job.waypoints[k].size() == n ? job.waypoints[k][i] : job.waypoints[k][0];
                    r.did_contact = collided[row] != 0;
                    r.outcome_is_valid = true;
                    r.microsteps = micro[row];
                    r.resolver_iterations = resolver[row];
                    r.error_flags = errors[row];
                }
        }
        return results;
    }
    /* ReverseSimulateRobots (SPCS:806-822) == forward simulation (SPCS:838-841) */
    std::vector<SimulationResult> ReverseSimulateRobots(const RobotDescription& immutable_robot,
                                                        const std::vector<Configuration>& start_positions,
                                                        const std::vector<Configuration>& target_positions,
                                                        bool allow_contacts, const DisplayFn& display_fn = {}) {
        (void)display_fn;
        return Simulate(immutable_robot, start_positions, target_positions, allow_contacts, true);
    }
    /* ForwardSimulateRobot (SPCS:824-829) as a batch of one */
    SimulationResult ForwardSimulateRobot(const RobotDescription& immutable_robot, const Configuration& start_position,
                                          const Configuration& target_position, bool allow_contacts) {
        return Simulate(immutable_robot, {start_position}, {target_position}, allow_contacts, false).front();
    }
    /* ForwardSimulateRobot(..., trace, enable_tracing, display_fn) (SPCS:824-829): the
     * traced kernel records the trace; without enable_tracing this is the call above */
    SimulationResult ForwardSimulateRobot(const RobotDescription& immutable_robot, const Configuration& start_position,
                                          const Configuration& target_position, bool allow_contacts,
                                          ForwardSimulationStepTrace& trace, bool enable_tracing,
                                          const DisplayFn& display_fn = {}, uint32_t config_capacity = 4096) {
        (void)display_fn;
        if (!enable_tracing) return ForwardSimulateRobot(immutable_robot, start_position, target_position, allow_contacts);
        SetRobot(immutable_robot);
        const size_t W = (size_t)immutable_robot.ConfigurationWidth(), D = (size_t)immutable_robot.NumDofs();
        if (start_position.size() != W || target_position.size() != W)
            throw std::invalid_argument("configuration has the wrong width");
        const uint32_t step_cap = forward_steps_, cfg_cap = config_capacity;
        std::vector<double> inputs((size_t)step_cap * 2 * D), configs((size_t)cfg_cap * W), out(W);
        std::vector<uint32_t> micro(step_cap), tags((size_t)cfg_cap * 3);
        uint32_t num_steps = 0, num_configs = 0, microsteps = 0, resolver = 0, errors = 0;
        uint8_t collided = 0;
        fks_trace t{step_cap, cfg_cap, inputs.data(), micro.data(), configs.data(), tags.data(), &num_steps, &num_configs};
        check(fks_forward_simulate_traced(ctx_, start_position.data(), 1, target_position.data(), 1, allow_contacts ? 1 : 0,
                                          out.data(), &collided, &microsteps, &resolver, &errors, &t),
              ctx_, "ForwardSimulateRobot");
        trace.truncated = trace.truncated || num_steps > step_cap || num_configs > cfg_cap;
        const size_t base = trace.resolver_steps.size(); /* the reference appends to the caller's trace */
        for (uint32_t k = 0; k < num_steps && k < step_cap; ++k) {
            ForwardSimulationResolverTrace rs;
            rs.control_input.assign(inputs.begin() + (size_t)k * 2 * D, inputs.begin() + (size_t)k * 2 * D + D);
            rs.control_input_step.assign(inputs.begin() + (size_t)k * 2 * D + D, inputs.begin() + (size_t)(k + 1) * 2 * D);
            trace.resolver_steps.push_back(std::move(rs));
        }
        int64_t last_step = -1, last_micro = -1;
        for (uint32_t k = 0; k < num_configs && k < cfg_cap; ++k) {
            const uint32_t st = tags[3 * k], mi = tags[3 * k + 1];
            if (base + st >= trace.resolver_steps.size()) break;
            ForwardSimulationResolverTrace& rs = trace.resolver_steps[base + st];
            if ((int64_t)st != last_step || (int64_t)mi != last_micro) rs.contact_resolver_steps.emplace_back();
            last_step = st;
            last_micro = mi;
            rs.contact_resolver_steps.back().contact_resolution_steps.emplace_back(configs.begin() + (size_t)k * W,
                                                                                   configs.begin() + (size_t)(k + 1) * W);
            rs.contact_resolver_steps.back().kinds.push_back(tags[3 * k + 2]);
        }
        SimulationResult r;
        r.result_config = out;
        r.target_config = target_position;
        r.did_contact = collided != 0;
        r.microsteps = microsteps;
        r.resolver_iterations = resolver;
        r.error_flags = errors;
        return r;
    }
    /* ReverseSimulateRobot (SPCS:831-836) */
    SimulationResult ReverseSimulateRobot(const RobotDescription& immutable_robot, const Configuration& start_position,
                                          const Configuration& target_position, bool allow_contacts) {
        return Simulate(immutable_robot, {start_position}, {target_position}, allow_contacts, true).front();
    }

    /* CheckConfigCollision (SPCS:1398-1416) */
    bool CheckConfigCollision(const RobotDescription& immutable_robot, const Configuration& config, double inflation_ratio) {
        return CheckConfigCollisions(immutable_robot, {config}, inflation_ratio).front();
    }
    /* the same check for a batch of configurations in one launch */
    std::vector<bool> CheckConfigCollisions(const RobotDescription& immutable_robot, const std::vector<Configuration>& configs,
                                            double inflation_ratio) {
        SetRobot(immutable_robot);
        const size_t W = (size_t)immutable_robot.ConfigurationWidth();
        const size_t n = configs.size();
        std::vector<double> c(n * W);
        for (size_t i = 0; i < n; ++i) {
            if (configs[i].size() != W) throw std::invalid_argument("configuration has the wrong width");
            std::copy(configs[i].begin(), configs[i].end(), c.begin() + i * W);
        }
        std::vector<uint8_t> collided(n);
        dev_.check_configs(c.data(), n, inflation_ratio, collided.data(), nullptr, "CheckConfigCollision");
        return std::vector<bool>(collided.begin(), collided.end());
    }

    fks_context* context() { return ctx_; }

  private:
    DeviceSet dev_;
    uint64_t select_seed_ = 0, select_calls_ = 0; /* SelectStates' draw seeds (SelectDrawSeed) */
    fks_context* ctx_ = nullptr; /* devices[0] */
    std::vector<unsigned char> robot_fingerprint_; /* the robot set last (RobotDescription::Fingerprint) */
    uint32_t forward_steps_ = 1; /* controller steps per simulation (SPCS:856): the trace's step capacity */
    double resolution_ = 0.0;
    std::string frame_ = "world";
    std::mt19937_64 rng_;

    /* RobotDescription is a mutable value the caller owns, so the robot set last is
     * recognised by content, never by address (a freed robot's address may be reused) */
    void SetRobot(const RobotDescription& robot) {
        std::vector<unsigned char> fp = robot.Fingerprint();
        if (!robot_fingerprint_.empty() && fp == robot_fingerprint_) return;
        robot_fingerprint_.clear();
        const fks_robot_desc d = robot.View();
        dev_.set_robot(d);
        robot_fingerprint_ = std::move(fp);
    }

    std::vector<SimulationResult> Simulate(const RobotDescription& robot, const std::vector<Configuration>& starts,
                                           const std::vector<Configuration>& targets, bool allow_contacts, bool reverse) {
        /* SPCS:792: one target per particle or one shared target */
        if (!starts.empty() && targets.size() != 1 && targets.size() != starts.size())
            throw std::invalid_argument("target_positions must hold 1 or start_positions.size() configurations");
        SetRobot(robot);
        const size_t W = (size_t)robot.ConfigurationWidth();
        const size_t n = starts.size();
        std::vector<double> s(n * W), t(targets.size() * W), out(n * W);
        for (size_t i = 0; i < n; ++i) {
            if (starts[i].size() != W) throw std::invalid_argument("start configuration has the wrong width");
            std::copy(starts[i].begin(), starts[i].end(), s.begin() + i * W);
        }
        for (size_t i = 0; i < targets.size(); ++i) {
            if (targets[i].size() != W) throw std::invalid_argument("target configuration has the wrong width");
            std::copy(targets[i].begin(), targets[i].end(), t.begin() + i * W);
        }
        std::vector<uint8_t> collided(n);
        std::vector<uint32_t> micro(n), resolver(n), errors(n);
        dev_.simulate(reverse, s.data(), n, t.data(), targets.size(), allow_contacts, out.data(), collided.data(), micro.data(),
                      resolver.data(), errors.data(), reverse ? "ReverseSimulateRobots" : "ForwardSimulateRobots");
        std::vector<SimulationResult> results(n);
        for (size_t i = 0; i < n; ++i) {
            SimulationResult& r = results[i];
            r.result_config.assign(out.begin() + i * W, out.begin() + (i + 1) * W);
            r.target_config = targets.size() == n ? targets[i] : targets[0];
            r.did_contact = collided[i] != 0;
            r.outcome_is_valid = true;
            r.microsteps = micro[i];
            r.resolver_iterations = resolver[i];
            r.error_flags = errors[i];
        }
        return results;
    }
};

/* fast_kinematic_simulator::Make{SE2,SE3,Linked}Simulator (FKS.cpp:4-71).  Without a device
 * argument the simulator runs on every visible MI355X (batches sharded by particle); `device`
 * or `devices` select them explicitly. */
inline std::shared_ptr<HipParticleContactSimulator> MakeSimulator(const fks_environment& environment, const fks_solver_params& solver_config,
                                                                  double simulation_controller_frequency, uint64_t prng_seed,
                                                                  int32_t debug_level, const std::vector<int32_t>& devices) {
    return std::make_shared<HipParticleContactSimulator>(environment, solver_config, simulation_controller_frequency, prng_seed,
                                                         debug_level, devices);
}
#define FKS_WRAPPER_FACTORY(NAME)                                                                                                 \
    inline std::shared_ptr<HipParticleContactSimulator> NAME(const fks_environment& environment, const fks_solver_params& solver_config, \
                                                             double simulation_controller_frequency, uint64_t prng_seed,        \
                                                             int32_t debug_level, const std::vector<int32_t>& devices) {       \
        return MakeSimulator(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level, devices);     \
    }                                                                                                                            \
    inline std::shared_ptr<HipParticleContactSimulator> NAME(const fks_environment& environment, const fks_solver_params& solver_config, \
                                                             double simulation_controller_frequency, uint64_t prng_seed,        \
                                                             int32_t debug_level, int32_t device) {                            \
        return MakeSimulator(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level,               \
                             std::vector<int32_t>{device});                                                                     \
    }                                                                                                                            \
    inline std::shared_ptr<HipParticleContactSimulator> NAME(const fks_environment& environment, const fks_solver_params& solver_config, \
                                                             double simulation_controller_frequency, uint64_t prng_seed,        \
                                                             int32_t debug_level) {                                             \
        return MakeSimulator(environment, solver_config, simulation_controller_frequency, prng_seed, debug_level,               \
                             AllVisibleDevices());                                                                              \
    }
FKS_WRAPPER_FACTORY(MakeSE2Simulator)
FKS_WRAPPER_FACTORY(MakeSE3Simulator)
FKS_WRAPPER_FACTORY(MakeLinkedSimulator)
#undef FKS_WRAPPER_FACTORY

}  // namespace fks

#endif
