/*
 * SummarizeClusters of both C++ layers against the C-ABI entries they wrap, on a scene read from a
 * file:
 *
 *   summary_interface_test <scene file>
 *
 * The scene (written by tests/test_summary_interface.py: the SE(2) workload cfg1) is
 * cluster_interface_test.cpp's: planner_interface_test.cpp's SE(2) scene followed by
 *
 *   groups <G> <count of thresholds> <thresholds>
 *   per group: <n> and its n configurations
 *
 * Three simulators are made over the one environment: the planner drop-in
 * (fast_kinematic_simulator::MakeSE2Simulator, its method reached through dynamic_cast as a
 * planner does), the plain class (fks::HipParticleContactSimulator over the robot's
 * HipDescription()), and a second plain one whose context takes fks_summarize_clusters_ctx.  For
 * every threshold the groups are labelled by fks_cluster_configs; with one target per group (its
 * first configuration; a start for an empty group) every array of both classes' SummarizeClusters and of both static
 * SummarizeClustersHost is compared bitwise with the C-ABI call's arrays and with
 * fks_summarize_clusters, and once more without targets; the call index and statistics of the
 * drop-in must not move.  The program also checks that the case decides something: some cluster
 * of several members has some of them within reach and some not.
 * Exit status 0 = identical, 1 = a difference (printed), 3 = no GPU.
 *
 *   build:  python -c "from fast_kinematic_simulator_amd.build import build_summary_test; build_summary_test()"
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "fast_kinematic_simulator_amd/fast_kinematic_simulator.hpp"

namespace upc = uncertainty_planning_core;
using fks_planner_types::Isometry3d;
using fks_planner_types::Vector3d;
using fks_planner_types::Vector4d;
typedef std::remove_cv<std::remove_reference<decltype(*std::declval<simple_robot_models::PointSphereGeometry>().Geometry())>::type>::type Points;
typedef tnuva_robot_models::TnuvaSE2Robot<upc::PRNG> Robot;
typedef simple_particle_contact_simulator::HipParticleContactSimulator<Robot, upc::SE2Config, upc::PRNG, upc::SE2ConfigAlloc> DropIn;
typedef simple_simulator_interface::SimulatorInterface<upc::SE2Config, upc::PRNG, upc::SE2ConfigAlloc> Interface;
typedef std::vector<upc::SE2Config, upc::SE2ConfigAlloc> Configs;

struct Reader {
    std::ifstream in;
    explicit Reader(const char* path) : in(path) {
        if (!in) throw std::runtime_error("cannot open scene file");
    }
    std::string word() {
        std::string w;
        if (!(in >> w)) throw std::runtime_error("truncated scene file");
        return w;
    }
    double num() { return std::strtod(word().c_str(), nullptr); }
    int64_t integer() { return std::strtoll(word().c_str(), nullptr, 10); }
    void expect(const char* tag) {
        const std::string w = word();
        if (w != tag) throw std::runtime_error("scene file: expected " + std::string(tag) + ", got " + w);
    }
    std::vector<double> nums(size_t n) {
        std::vector<double> v(n);
        for (double& x : v) x = num();
        return v;
    }
};

static int g_bad = 0;
static void differs(const char* what, size_t with_targets) {
    if (g_bad++ < 12) std::printf("%s differs (targets: %zu)\n", what, with_targets);
}
static bool same(const std::vector<double>& a, const double* b) { return std::memcmp(a.data(), b, a.size() * sizeof(double)) == 0; }

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scene>\n", argv[0]);
        return 2;
    }
    try {
        Reader r(argv[1]);
        r.expect("family");
        if (r.word() != "se2") throw std::runtime_error("the summary program reads an SE(2) scene");
        r.expect("frequency");
        const double frequency = r.num();
        r.expect("seed");
        const uint64_t seed = (uint64_t)r.integer();
        r.expect("allow");
        const bool allow = r.integer() != 0;
        r.expect("solver");
        fast_kinematic_simulator::SolverParameters solver;
        solver.forward_simulation_time = r.num();
        solver.simulation_shortcut_distance = r.num();
        solver.environment_collision_check_tolerance = r.num();
        solver.resolve_correction_step_scaling_decay_rate = r.num();
        solver.resolve_correction_initial_step_size = r.num();
        solver.resolve_correction_min_step_scaling = r.num();
        solver.max_resolver_iterations = (uint32_t)r.integer();
        solver.resolve_correction_step_scaling_decay_iterations = (uint32_t)r.integer();
        solver.failed_resolves_end_motion = r.integer() != 0;
        r.expect("env");
        const double resolution = r.num();
        const std::vector<double> origin = r.nums(12);
        int64_t cells[3];
        for (int64_t& c : cells) c = r.integer();
        const int64_t nobs = r.integer();
        std::vector<simulator_environment_builder::OBSTACLE_CONFIG> obstacles;
        for (int64_t k = 0; k < nobs; ++k) {
            const std::vector<double> pose = r.nums(12), ext = r.nums(3);
            obstacles.emplace_back((uint32_t)r.integer(), fks_ext::iso_from_row_major34(pose.data()), Vector3d(ext[0], ext[1], ext[2]));
        }
        const simulator_environment_builder::EnvironmentComponents E =
            simulator_environment_builder::BuildCompleteEnvironment(obstacles, resolution, origin.data(), cells);
        /* the TnuvaSE2Robot: position and rotation weight, points, the 18 gains of its config */
        const double pw = r.num(), rw = r.num();
        auto pts = std::make_shared<Points>();
        for (int64_t i = r.integer(); i > 0; --i) {
            const std::vector<double> v = r.nums(4);
            pts->push_back(Vector4d(v[0], v[1], v[2], v[3]));
        }
        const simple_robot_models::PointSphereGeometry geometry(simple_robot_models::PointSphereGeometry::POINTS, pts);
        const std::vector<double> c = r.nums(18);
        const tnuva_robot_models::AXIS_ROBOT_CONFIG cfg(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11], c[12],
                                                        c[13], c[14], c[15], c[16], c[17]);
        const auto robot = std::make_shared<Robot>(upc::SE2Config(0.0, 0.0, 0.0), pw, rw, "body", geometry, cfg);
        const std::shared_ptr<Interface::BaseRobotType> base = robot;
        const size_t W = 3;
        auto read_configs = [&](size_t count, Configs& typed, std::vector<fks::Configuration>& flat) {
            for (size_t i = 0; i < count; ++i) {
                flat.push_back(r.nums(W));
                typed.push_back(robot->FromFlat(flat.back().data()));
            }
        };
        Configs starts, ignored;
        std::vector<fks::Configuration> flat_starts, flat_ignored;
        r.expect("starts");
        read_configs((size_t)r.integer(), starts, flat_starts);
        r.expect("targets");
        read_configs((size_t)r.integer(), ignored, flat_ignored);
        (void)allow;
        r.expect("groups");
        const size_t G = (size_t)r.integer();
        const std::vector<double> thresholds = r.nums((size_t)r.integer());
        std::vector<Configs> groups(G);
        std::vector<std::vector<fks::Configuration>> flat_groups(G);
        for (size_t g = 0; g < G; ++g) read_configs((size_t)r.integer(), groups[g], flat_groups[g]);

        /* the three simulators: drop-in, plain class, and the context of the C-ABI call */
        const upc::SE2SimulatorPtr drop_in_sim = fast_kinematic_simulator::MakeSE2Simulator(
            E.GetEnvironment(), E.GetEnvironmentSDF(), E.GetSurfaceNormalsGrid(), solver, frequency, seed, 0, {0});
        DropIn* drop_in = dynamic_cast<DropIn*>(drop_in_sim.get());
        if (!drop_in) throw std::runtime_error("the factory did not return the HIP simulator");
        std::vector<float> sdf_storage;
        const fks_environment env =
            simulator_environment_builder::ToFksEnvironment(E.GetEnvironment(), E.GetEnvironmentSDF(), E.GetSurfaceNormalsGrid(), sdf_storage);
        const fks::RobotDescription& description = robot->HipDescription();
        fks::HipParticleContactSimulator plain_sim(env, solver.ToFks(), frequency, seed, 0, {0});
        fks::HipParticleContactSimulator abi_sim(env, solver.ToFks(), frequency, seed, 0, {0});
        const fks_robot_desc d = description.View();
        fks::check(fks_set_robot(abi_sim.context(), &d), abi_sim.context(), "fks_set_robot");
        const std::map<std::string, double> stats_before = drop_in_sim->GetStatistics();

        std::vector<fks::Configuration> flat_targets;
        Configs targets;
        for (size_t g = 0; g < G; ++g) {
            flat_targets.push_back(flat_groups[g].empty() ? flat_starts.at(0) : flat_groups[g][0]);
            targets.push_back(robot->FromFlat(flat_targets.back().data()));
        }
        const double reach = 0.3;
        fks::FlatClusterGroups twin_labels(flat_groups, W, false);
        bool decided = false;
        for (const double threshold : thresholds) {
            if (fks_cluster_configs(&d, twin_labels.configs.data(), twin_labels.begin.data(), G, threshold, nullptr, twin_labels.labels_ptr(),
                                    twin_labels.counts_ptr()) != FKS_OK)
                throw std::runtime_error("fks_cluster_configs failed");
            const std::vector<std::vector<uint32_t>> labels = twin_labels.result(false).labels;
            for (int with_targets = 1; with_targets >= 0; --with_targets) {
                const std::vector<fks::Configuration> ft = with_targets ? flat_targets : std::vector<fks::Configuration>();
                const Configs tt = with_targets ? targets : Configs();
                fks::FlatSummaryGroups abi(flat_groups, labels, ft, W, 3), twin(flat_groups, labels, ft, W, 3);
                fks::check(fks_summarize_clusters_ctx(abi_sim.context(), abi.configs.data(), abi.out.group_begin.data(), G, abi.labels.data(),
                                                      abi.targets_or_null(), reach, &abi.summary),
                           abi_sim.context(), "fks_summarize_clusters_ctx");
                if (fks_summarize_clusters(&d, twin.configs.data(), twin.out.group_begin.data(), G, twin.labels.data(), twin.targets_or_null(),
                                           reach, &twin.summary) != FKS_OK)
                    throw std::runtime_error("fks_summarize_clusters failed");
                const fks::ClusterSummaries& ref = abi.out;
                const fks::ClusterSummaries results[5] = {twin.out,
                                                          plain_sim.SummarizeClusters(description, flat_groups, labels, ft, reach),
                                                          drop_in->SummarizeClusters(base, groups, labels, tt, reach),
                                                          fks::HipParticleContactSimulator::SummarizeClustersHost(description, flat_groups, labels, ft, reach),
                                                          DropIn::SummarizeClustersHost(base, groups, labels, tt, reach)};
                const char* names[5] = {"host twin", "plain class", "drop-in", "plain class, host", "drop-in, host"};
                for (int k = 0; k < 5; ++k) {
                    const fks::ClusterSummaries& got = results[k];
                    if (got.width != W || got.var_width != 3 || got.group_begin != ref.group_begin || got.order != ref.order ||
                        got.count != ref.count || got.begin != ref.begin || got.reached != ref.reached ||
                        got.reached.size() != (with_targets ? ref.count.size() : 0) || got.members.size() != ref.members.size() ||
                        !same(got.members, ref.members.data()) || got.expectation.size() != ref.expectation.size() ||
                        !same(got.expectation, ref.expectation.data()) || got.variances.size() != ref.variances.size() ||
                        !same(got.variances, ref.variances.data()) || got.variance.size() != ref.variance.size() ||
                        !same(got.variance, ref.variance.data()))
                        differs(names[k], (size_t)with_targets);
                }
                if (with_targets)
                    for (size_t row = 0; row < ref.count.size(); ++row)
                        decided = decided || (ref.count[row] >= 2 && ref.reached[row] >= 1 && ref.reached[row] < ref.count[row]);
            }
            std::printf("threshold %g: %zu groups, %d differences so far\n", threshold, G, g_bad);
        }
        if (!decided) {
            std::printf("the case decides too little: no cluster of several members is partly within reach\n");
            ++g_bad;
        }
        if (drop_in_sim->GetStatistics() != stats_before) {
            std::printf("the statistics moved\n");
            ++g_bad;
        }
        std::printf("summaries compared, %d differences\n", g_bad);
        return g_bad ? 1 : 0;
    } catch (const fks::SimulatorError& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status() == FKS_ERR_NO_DEVICE ? 3 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
