/*
 * ForwardSimulateRobotsUnderPolicy of both C++ layers against the C-ABI call they wrap, on a
 * scene read from a file:
 *
 *   policy_interface_test <scene file>
 *
 * The scene (written by tests/test_policy_interface.py from tests/policy_cases.py: the SE(2)
 * workload cfg1 with case 1's starts and table) is planner_interface_test.cpp's SE(2) scene
 * (the TnuvaSE2Robot's constructor arguments, the obstacles for BuildCompleteEnvironment, the
 * solver parameters, starts, targets) followed by
 *
 *   policy <M> <max_legs> <terminal_distance>
 *   <M keys> <M targets> <M terminal flags>
 *   max_distances <count> <values>
 *
 * Three simulators are made over the one environment with the scene's seed: the planner drop-in
 * (fast_kinematic_simulator::MakeSE2Simulator, its method reached through dynamic_cast as a
 * planner does), the plain class (fks::HipParticleContactSimulator over the robot's
 * HipDescription()), and a second plain one whose context takes fks_forward_simulate_policy.
 * For every max_distance in turn, all three roll the starts out (so they stand at the same call
 * index throughout) and every result of the two classes is compared bitwise with the C-ABI
 * call's arrays, their statistics with its context's; the static PolicySelect of both classes
 * must give the roll-out's first selection.  The program also checks that the case decides
 * something: stops at three or more different legs, leg 0 among them, an entry past the first 64
 * chosen, the tie of entries 10 and 66 met and resolved to 10, contacts in every leg.
 * Exit status 0 = identical, 1 = a difference (printed), 3 = no GPU.
 *
 *   build:  python -c "from fast_kinematic_simulator_amd.build import build_policy_test; build_policy_test()"
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

static bool same_bytes(const std::vector<double>& a, const double* b) { return std::memcmp(a.data(), b, a.size() * sizeof(double)) == 0; }

static int g_bad = 0;
static void differs(const char* what, size_t k, size_t i) {
    if (g_bad++ < 12) std::printf("%s: leg or selection %zu, particle %zu\n", what, k, i);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scene>\n", argv[0]);
        return 2;
    }
    try {
        Reader r(argv[1]);
        r.expect("family");
        if (r.word() != "se2") throw std::runtime_error("the policy program reads an SE(2) scene");
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
        r.expect("policy");
        const size_t M = (size_t)r.integer(), K = (size_t)r.integer(), n = starts.size();
        DropIn::PolicyTable policy;
        fks::PolicyTable plain_policy;
        policy.terminal_distance = plain_policy.terminal_distance = r.num();
        read_configs(M, policy.keys, plain_policy.keys);
        read_configs(M, policy.targets, plain_policy.targets);
        for (size_t i = 0; i < M; ++i) policy.terminal.push_back(r.integer() != 0);
        plain_policy.terminal = policy.terminal;
        r.expect("max_distances");
        const std::vector<double> max_distances = r.nums((size_t)r.integer());

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
        {
            const fks_robot_desc d = description.View();
            fks::check(fks_set_robot(abi_sim.context(), &d), abi_sim.context(), "fks_set_robot");
        }
        std::vector<double> s;
        for (const auto& q : flat_starts) s.insert(s.end(), q.begin(), q.end());

        for (const double max_distance : max_distances) {
            policy.max_distance = plain_policy.max_distance = max_distance;
            const fks::FlatPolicyTable flat(plain_policy, W);
            std::vector<double> q(K * n * W), dist((K + 1) * n);
            std::vector<uint8_t> collided(K * n);
            std::vector<uint32_t> micro(K * n), resolver(K * n), errors(K * n), choice((K + 1) * n), legs(n);
            fks::check(fks_forward_simulate_policy(abi_sim.context(), s.data(), n, &flat.table, K, allow ? 1 : 0, q.data(), collided.data(),
                                                   micro.data(), resolver.data(), errors.data(), choice.data(), dist.data(), legs.data()),
                       abi_sim.context(), "fks_forward_simulate_policy");
            const fks::PolicyRollout plain = plain_sim.ForwardSimulateRobotsUnderPolicy(description, flat_starts, plain_policy, K, allow);
            const DropIn::PolicyRollout typed = drop_in->ForwardSimulateRobotsUnderPolicy(base, starts, policy, K, allow);
            if (plain.results.size() != K || typed.results.size() != K || plain.choices.size() != K + 1 || typed.choices.size() != K + 1 ||
                plain.distances.size() != K + 1 || typed.distances.size() != K + 1 || plain.legs_run.size() != n ||
                typed.legs_run.size() != n || drop_in->LastMicrosteps().size() != K * n ||
                drop_in->LastResolverIterations().size() != K * n || drop_in->LastParticleErrors().size() != K * n)
                throw std::runtime_error("a roll-out of the wrong shape");

            /* what the case decides (on the C-ABI call's arrays) */
            std::set<uint32_t> stop_legs;
            bool high = false, ten = false;
            std::vector<size_t> contacts(K, 0);
            for (size_t i = 0; i < n; ++i)
                if (legs[i] < K) stop_legs.insert(legs[i]);
            for (size_t k = 0; k <= K; ++k)
                for (size_t i = 0; i < n; ++i) {
                    const size_t row = k * n + i;
                    if (choice[row] >= FKS_POLICY_LOST) continue;
                    const uint32_t entry = choice[row] & ~FKS_POLICY_ARRIVED;
                    high = high || entry >= 64;
                    ten = ten || entry == 10; /* entries 10 and 66 hold one key: every choice of 10 met the tie */
                    if (entry == 66) differs("the duplicate entry 66 was chosen", k, i);
                    if (k < K && collided[row]) contacts[k]++;
                }
            if (stop_legs.size() < 3 || !stop_legs.count(0) || !high || !ten) {
                std::printf("max_distance %g: the case decides too little (%zu stop legs, leg 0 %d, entry >= 64 %d, entry 10 %d)\n",
                            max_distance, stop_legs.size(), (int)stop_legs.count(0), high ? 1 : 0, ten ? 1 : 0);
                ++g_bad;
            }
            for (size_t k = 0; k < K; ++k)
                if (contacts[k] == 0) {
                    std::printf("max_distance %g: no contact in leg %zu\n", max_distance, k);
                    ++g_bad;
                }

            /* both classes against the arrays */
            for (size_t k = 0; k <= K; ++k)
                for (size_t i = 0; i < n; ++i) {
                    const size_t row = k * n + i;
                    if (plain.choices[k][i] != choice[row] || std::memcmp(&plain.distances[k][i], &dist[row], sizeof(double)) != 0)
                        differs("plain class, selection", k, i);
                    if (typed.choices[k][i] != choice[row] || std::memcmp(&typed.distances[k][i], &dist[row], sizeof(double)) != 0)
                        differs("drop-in, selection", k, i);
                    if (k == K) continue;
                    const bool ran = k < legs[i];
                    const fks::SimulationResult& a = plain.results[k][i];
                    if (!same_bytes(a.result_config, q.data() + row * W) || a.did_contact != (collided[row] != 0) || !a.outcome_is_valid ||
                        a.microsteps != micro[row] || a.resolver_iterations != resolver[row] || a.error_flags != errors[row])
                        differs("plain class, result", k, i);
                    if (a.target_config != (ran ? plain_policy.targets[choice[row] & ~FKS_POLICY_ARRIVED] : a.result_config))
                        differs("plain class, target_config", k, i);
                    const Interface::SimulationResult& b = typed.results[k][i];
                    if (!same_bytes(robot->ToFlat(b.result_config), q.data() + row * W) || b.did_contact != (collided[row] != 0) ||
                        !b.outcome_is_valid || drop_in->LastMicrosteps()[row] != micro[row] ||
                        drop_in->LastResolverIterations()[row] != resolver[row] || drop_in->LastParticleErrors()[row] != errors[row])
                        differs("drop-in, result", k, i);
                    const std::vector<double> target = robot->ToFlat(b.target_config);
                    if (!same_bytes(target, ran ? plain_policy.targets[choice[row] & ~FKS_POLICY_ARRIVED].data() : q.data() + row * W))
                        differs("drop-in, target_config", k, i);
                }
            for (size_t i = 0; i < n; ++i)
                if (plain.legs_run[i] != legs[i] || typed.legs_run[i] != legs[i]) differs("legs_run", 0, i);
            const std::vector<std::pair<std::string, double>> abi_stats = abi_sim.GetStatistics();
            if (plain_sim.GetStatistics() != abi_stats ||
                drop_in_sim->GetStatistics() != std::map<std::string, double>(abi_stats.begin(), abi_stats.end())) {
                std::printf("max_distance %g: statistics differ\n", max_distance);
                ++g_bad;
            }
            /* the static selections: the roll-out's first */
            const fks::PolicySelection sel_plain = fks::HipParticleContactSimulator::PolicySelect(description, plain_policy, flat_starts);
            const fks::PolicySelection sel_typed = DropIn::PolicySelect(base, policy, starts);
            for (size_t i = 0; i < n; ++i) {
                if (sel_plain.choices[i] != choice[i] || std::memcmp(&sel_plain.distances[i], &dist[i], sizeof(double)) != 0)
                    differs("plain class, PolicySelect", 0, i);
                if (sel_typed.choices[i] != choice[i] || std::memcmp(&sel_typed.distances[i], &dist[i], sizeof(double)) != 0)
                    differs("drop-in, PolicySelect", 0, i);
            }
            std::printf("max_distance %g: %zu particles, %zu legs, stops at %zu legs, %d differences so far\n", max_distance, n, K,
                        stop_legs.size(), g_bad);
        }
        std::printf("roll-outs compared, %d differences\n", g_bad);
        return g_bad ? 1 : 0;
    } catch (const fks::SimulatorError& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status() == FKS_ERR_NO_DEVICE ? 3 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
