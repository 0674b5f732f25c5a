/*
 * ForwardSimulateRobotsAlongPath (include/fast_kinematic_simulator_amd/
 * hip_particle_contact_simulator.hpp) against the chain of ForwardSimulateRobots calls it
 * replaces: an SE(2) bar among three boxes, built in code, a batch of particles along a
 * path of three shared waypoints and along one of per-particle waypoints.  A second simulator
 * made with the same seed runs the chained calls; every result is compared bitwise, and so are
 * the statistics.  Exit status 0 = identical, 1 = a difference (printed), 3 = no GPU.
 *
 * FKS_TEST_DEVICES ("0,0") and FKS_TEST_SHARD (1 = shard every batch) select the device list,
 * as in planner_interface_test.cpp; the comparison must hold for any of them.
 *
 *   build:  python -c "from fast_kinematic_simulator_amd.build import build_cpp_program; \
 *                      build_cpp_program('tests/cpp/path_interface_test.cpp', 'path_interface_test')"
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "fast_kinematic_simulator_amd/hip_particle_contact_simulator.hpp"

static std::vector<int32_t> test_devices() {
    const char* e = std::getenv("FKS_TEST_DEVICES");
    if (!e || !e[0]) return {0};
    std::vector<int32_t> d;
    std::stringstream ss(e);
    std::string item;
    while (std::getline(ss, item, ',')) d.push_back((int32_t)std::atoi(item.c_str()));
    return d;
}

static fks_dof_controller controller(double kp, double vmax) {
    fks_dof_controller c{};
    c.kp = kp;
    c.ki = 0.1;
    c.kd = 0.01;
    c.integral_clamp = 1.0;
    c.velocity_limit = vmax;
    c.max_sensor_noise = 0.001;
    c.max_actuator_proportional_noise = 0.1;
    c.max_actuator_minimum_noise = 0.001;
    return c;
}

/* a bar of 0.6 x 0.2 m sampled every 5 cm, in the plane z = 0 */
static fks::RobotDescription bar_robot() {
    fks::RobotDescription r;
    r.type = FKS_ROBOT_SE2;
    r.num_links = 1;
    r.num_dofs = 3;
    std::vector<double> pts;
    for (int i = 0; i <= 12; ++i)
        for (int j = 0; j <= 4; ++j) {
            pts.push_back(-0.3 + 0.05 * i);
            pts.push_back(-0.1 + 0.05 * j);
            pts.push_back(0.0);
            pts.push_back(1.0);
        }
    r.AddGeometry(0, pts);
    r.controllers = {controller(2.0, 1.0), controller(2.0, 1.0), controller(2.0, 1.5)};
    r.distance_weights = {1.0, 0.5};
    return r;
}

static fks_obstacle make_box(uint32_t id, double x, double y, double hx, double hy) {
    fks_obstacle b{};
    const double pose[12] = {1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, 0};
    for (int k = 0; k < 12; ++k) b.pose[k] = pose[k];
    b.extents[0] = hx;
    b.extents[1] = hy;
    b.extents[2] = 0.25;
    b.object_id = id;
    return b;
}

static int differences(const char* what, const std::vector<std::vector<fks::SimulationResult>>& path,
                       const std::vector<std::vector<fks::SimulationResult>>& chain) {
    int bad = 0;
    if (path.size() != chain.size()) {
        std::printf("%s: %zu legs against %zu\n", what, path.size(), chain.size());
        return 1;
    }
    for (size_t k = 0; k < path.size(); ++k) {
        if (path[k].size() != chain[k].size()) {
            std::printf("%s leg %zu: %zu results against %zu\n", what, k, path[k].size(), chain[k].size());
            return bad + 1;
        }
        for (size_t i = 0; i < path[k].size(); ++i) {
            const fks::SimulationResult &a = path[k][i], &b = chain[k][i];
            const bool same = a.result_config.size() == b.result_config.size() &&
                              std::memcmp(a.result_config.data(), b.result_config.data(), a.result_config.size() * sizeof(double)) == 0 &&
                              a.target_config == b.target_config && a.did_contact == b.did_contact &&
                              a.outcome_is_valid == b.outcome_is_valid && a.microsteps == b.microsteps &&
                              a.resolver_iterations == b.resolver_iterations && a.error_flags == b.error_flags;
            if (!same) {
                if (bad < 8)
                    std::printf("%s leg %zu particle %zu: (%a %a %a) contact %d micro %u against (%a %a %a) contact %d micro %u\n", what,
                                k, i, a.result_config[0], a.result_config[1], a.result_config[2], a.did_contact ? 1 : 0, a.microsteps,
                                b.result_config[0], b.result_config[1], b.result_config[2], b.did_contact ? 1 : 0, b.microsteps);
                ++bad;
            }
        }
    }
    return bad;
}

int main() {
    const fks_obstacle boxes[3] = {make_box(1, 2.0, 2.0, 0.4, 0.4), make_box(2, 1.0, 3.0, 0.3, 0.5), make_box(3, 3.0, 1.0, 0.5, 0.3)};
    const double origin[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.25};
    const int64_t cells[3] = {64, 64, 8};
    fks_env_handle* env_handle = nullptr;
    fks::check(fks_env_build(boxes, 3, 0.0625, origin, cells, &env_handle), nullptr, "fks_env_build");
    fks_environment env;
    fks::check(fks_env_view(env_handle, &env), nullptr, "fks_env_view");

    const fks::RobotDescription robot = bar_robot();
    fks_solver_params params = fks::GetDefaultSolverParameters();
    params.forward_simulation_time = 2.0;
    const double frequency = 25.0; /* 50 controller steps per leg */
    const uint64_t seed = 20240611;
    const size_t n = 48;
    int status = 0;
    try {
        const std::vector<int32_t> devices = test_devices();
        auto path_sim = fks::MakeSE2Simulator(env, params, frequency, seed, 0, devices);
        auto chain_sim = fks::MakeSE2Simulator(env, params, frequency, seed, 0, devices);
        if (const char* e = std::getenv("FKS_TEST_SHARD")) {
            if (e[0]) {
                path_sim->SetShardThreshold(std::strtoull(e, nullptr, 10));
                chain_sim->SetShardThreshold(std::strtoull(e, nullptr, 10));
            }
        }
        std::vector<fks::Configuration> starts;
        for (size_t i = 0; i < n; ++i)
            starts.push_back({0.6 + 0.01 * std::sin(0.7 * (double)i), 0.6 + 0.01 * std::cos(0.3 * (double)i), 0.05 * (double)(i % 7)});
        /* across the middle box, then past the other two: legs make contact, and without
         * contacts allowed they end early */
        const std::vector<std::vector<fks::Configuration>> shared = {{{3.4, 3.4, 1.0}}, {{0.6, 3.4, -1.0}}, {{3.4, 0.6, 2.0}}};
        std::vector<std::vector<fks::Configuration>> own(2, std::vector<fks::Configuration>(n));
        for (size_t k = 0; k < own.size(); ++k)
            for (size_t i = 0; i < n; ++i)
                own[k][i] = {0.5 + 3.0 * std::fabs(std::sin(1.3 * (double)(i + 17 * k))), 0.5 + 3.0 * std::fabs(std::cos(0.9 * (double)(i + 5 * k))),
                             -3.0 + 0.125 * (double)((i * 7 + k) % 48)};
        int bad = 0;
        size_t contacts = 0;
        const struct Case {
            const char* name;
            const std::vector<std::vector<fks::Configuration>>* waypoints;
            bool allow_contacts;
        } cases[] = {{"shared waypoints", &shared, true}, {"shared waypoints, no contacts", &shared, false}, {"own waypoints", &own, true}};
        for (const Case& c : cases) {
            /* both simulators stand at the same call index: they made the same number of calls */
            const auto path = path_sim->ForwardSimulateRobotsAlongPath(robot, starts, *c.waypoints, c.allow_contacts);
            std::fprintf(stderr, "%s: devices %zu sharded %d over %d\n", c.name, path_sim->Devices().size(),
                         path_sim->LastBatchSharded() ? 1 : 0, path_sim->LastBatchDevices());
            std::vector<std::vector<fks::SimulationResult>> chain;
            std::vector<fks::Configuration> q = starts;
            for (const auto& leg : *c.waypoints) {
                chain.push_back(chain_sim->ForwardSimulateRobots(robot, q, leg, c.allow_contacts));
                q.clear();
                for (const auto& r : chain.back()) q.push_back(r.result_config);
            }
            bad += differences(c.name, path, chain);
            for (const auto& leg : chain)
                for (const auto& r : leg) contacts += r.did_contact ? 1 : 0;
            if (path_sim->GetStatistics() != chain_sim->GetStatistics()) {
                std::printf("%s: statistics differ\n", c.name);
                ++bad;
            }
        }
        if (contacts == 0) {
            std::printf("no leg of the chain made contact: the scene checks nothing\n");
            ++bad;
        }
        std::printf("legs compared, %zu contacts in the chains, %d differences\n", contacts, bad);
        status = bad ? 1 : 0;
    } catch (const fks::SimulatorError& e) {
        std::fprintf(stderr, "%s\n", e.what());
        status = e.status() == FKS_ERR_NO_DEVICE ? 3 : 1;
    }
    fks_env_free(env_handle);
    return status;
}
