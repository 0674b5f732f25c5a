/*
 * SelectStates of both C++ layers against the C-ABI entries they wrap, on a scene read from a file:
 *
 *   select_interface_test <scene file>
 *
 * The scene (written by tests/test_select_interface.py: the SE(2) workload cfg1) is
 * planner_interface_test.cpp's SE(2) scene followed by
 *
 *   table <S> <member rows> <P> <J>
 *   per state: its key, weight, count and begin
 *   the member rows, then the J queries
 *
 * Three simulators are made over the one environment: the planner drop-in
 * (fast_kinematic_simulator::MakeSE2Simulator, its method reached through dynamic_cast as a planner
 * does), the plain class (fks::HipParticleContactSimulator over the robot's HipDescription()), and
 * a second plain one whose context takes fks_select_states_ctx.  Three selections in a row (the
 * third after ResetGenerators, which starts the draw seeds again) with the whole table, and one
 * with keys and weights alone: every array of both classes' SelectStates and of both static
 * SelectStatesHost is compared bitwise with the C-ABI call's arrays and with fks_select_states at
 * the seed fks::SelectDrawSeed names; the device-pointer form is called with no query, which
 * launches nothing and still takes a seed.  The statistics of the drop-in must not move.  The program also checks that the case decides something: some job is drawn, some copied
 * in order, and two selections with different seeds differ.
 * Exit status 0 = identical, 1 = a difference (printed), 3 = no GPU.
 *
 *   build:  python -c "from fast_kinematic_simulator_amd.build import build_select_test; build_select_test()"
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
static void differs(const char* what, int round) {
    if (g_bad++ < 12) std::printf("%s differs (selection %d)\n", what, round);
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
        if (r.word() != "se2") throw std::runtime_error("the selection program reads an SE(2) scene");
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
        r.expect("table");
        const size_t S = (size_t)r.integer(), rows = (size_t)r.integer();
        const uint32_t P = (uint32_t)r.integer();
        const size_t J = (size_t)r.integer();
        fks::StateTable table;
        for (size_t i = 0; i < S; ++i) {
            const std::vector<double> key = r.nums(W);
            table.keys.insert(table.keys.end(), key.begin(), key.end());
            table.weights.push_back(r.num());
            table.count.push_back((uint32_t)r.integer());
            table.begin.push_back((uint32_t)r.integer());
        }
        table.members = r.nums(rows * W);
        Configs queries;
        std::vector<fks::Configuration> flat_queries;
        read_configs(J, queries, flat_queries);
        fks::StateTable bare; /* keys and weights alone: nothing to draw from */
        bare.keys = table.keys;
        bare.weights = table.weights;

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
        const std::vector<double> flat = fks::HipParticleContactSimulator::FlatQueries(flat_queries, W);

        bool drawn = false, in_order = false;
        std::vector<uint32_t> first_source;
        uint64_t k = 0; /* selections since the generators were last reset */
        for (int round = 0; round < 4; ++round) {
            const fks::StateTable& tab = round == 3 ? bare : table;
            if (round == 2) {
                /* the device-pointer form with no query: nothing is launched, and the call takes seed 2 */
                fks_state_table none = tab.View(W);
                fks_state_selection nothing = {nullptr, nullptr, nullptr, nullptr};
                const uint64_t s_plain = plain_sim.SelectStates(description, none, nullptr, 0, P, nothing);
                const uint64_t s_drop = drop_in->SelectStates(base, none, nullptr, 0, P, nothing);
                if (s_plain != fks::SelectDrawSeed(seed, 2) || s_drop != s_plain) differs("the device-pointer form's seed", round);
                plain_sim.ResetGenerators(seed);
                drop_in->ResetGenerators(seed);
                k = 0;
            }
            const uint64_t draw_seed = fks::SelectDrawSeed(seed, k++);
            fks::FlatStateSelection abi(tab, J, P, W, draw_seed), twin(tab, J, P, W, draw_seed);
            const fks_state_table view = tab.View(W);
            fks::check(fks_select_states_ctx(abi_sim.context(), &view, flat.data(), J, P, draw_seed, &abi.selection), abi_sim.context(),
                       "fks_select_states_ctx");
            if (fks_select_states(&d, &view, flat.data(), J, P, draw_seed, &twin.selection) != FKS_OK)
                throw std::runtime_error("fks_select_states failed");
            const fks::StateSelection& ref = abi.out;
            const fks::StateSelection results[5] = {twin.out, plain_sim.SelectStates(description, tab, flat_queries, P),
                                                    drop_in->SelectStates(base, tab, queries, P),
                                                    fks::HipParticleContactSimulator::SelectStatesHost(description, tab, flat_queries, P, draw_seed),
                                                    DropIn::SelectStatesHost(base, tab, queries, P, draw_seed)};
            const char* names[5] = {"host twin", "plain class", "drop-in", "plain class, host", "drop-in, host"};
            for (int c = 0; c < 5; ++c) {
                const fks::StateSelection& got = results[c];
                if (got.width != W || got.particles != (round == 3 ? 0u : P) || got.draw_seed != draw_seed || got.choice != ref.choice ||
                    got.source != ref.source || got.choice.size() != J || got.source.size() != (round == 3 ? 0 : J * P) ||
                    got.distance.size() != J || !same(got.distance, ref.distance.data()) || got.starts.size() != ref.starts.size() ||
                    got.starts.size() != (round == 3 ? 0 : J * P * W) || !same(got.starts, ref.starts.data()))
                    differs(names[c], round);
            }
            if (round < 3)
                for (size_t j = 0; j < J; ++j) {
                    if (ref.choice[j] == FKS_STATE_NONE) continue;
                    (table.count[ref.choice[j]] == P ? in_order : drawn) = true;
                }
            if (round == 0) first_source = ref.source;
            if (round == 1 && ref.source == first_source) differs("the second selection's draw (it repeats the first)", round);
            if (round == 2 && ref.source != first_source) differs("the selection after ResetGenerators (it does not repeat the first)", round);
            std::printf("selection %d: %zu queries, %d differences so far\n", round, J, g_bad);
        }
        if (!drawn || !in_order) {
            std::printf("the case decides too little: drawn %d, in order %d\n", (int)drawn, (int)in_order);
            ++g_bad;
        }
        if (drop_in_sim->GetStatistics() != stats_before) {
            std::printf("the statistics moved\n");
            ++g_bad;
        }
        std::printf("selections compared, %d differences\n", g_bad);
        return g_bad ? 1 : 0;
    } catch (const fks::SimulatorError& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status() == FKS_ERR_NO_DEVICE ? 3 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
