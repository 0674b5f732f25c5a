/*
 * ForwardSimulateRobotsJobsAlongPaths (include/fast_kinematic_simulator_amd/
 * hip_particle_contact_simulator.hpp) against the sequence of ForwardSimulateRobotsAlongPath
 * calls it replaces: an SE(2) bar among three boxes, built in code, and four independent path
 * jobs of different lengths (an edge simulated forward across the middle box and back to its
 * particles' own starts, a few particles on one leg without contacts, an empty job of two legs,
 * a three-leg tour with per-particle waypoints).  A second simulator made with the same seed
 * issues the path calls one after the other; every result is compared bitwise, and so are the
 * statistics.  Exit status 0 = identical, 1 = a difference (printed), 3 = no GPU.
 *
 * FKS_TEST_DEVICES ("0,0") and FKS_TEST_SHARD (1 = shard every batch) select the device list,
 * as in planner_interface_test.cpp; the comparison must hold for any of them.
 *
 *   build:  python -c "from fast_kinematic_simulator_amd.build import build_path_jobs_test; build_path_jobs_test()"
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

typedef std::vector<std::vector<fks::SimulationResult>> PathResults; /* [leg][particle] */

static int differences(const std::vector<PathResults>& batch, const std::vector<PathResults>& sequence) {
    int bad = 0;
    if (batch.size() != sequence.size()) {
        std::printf("%zu jobs against %zu\n", batch.size(), sequence.size());
        return 1;
    }
    for (size_t j = 0; j < batch.size(); ++j) {
        if (batch[j].size() != sequence[j].size()) {
            std::printf("job %zu: %zu legs against %zu\n", j, batch[j].size(), sequence[j].size());
            return bad + 1;
        }
        for (size_t k = 0; k < batch[j].size(); ++k) {
            if (batch[j][k].size() != sequence[j][k].size()) {
                std::printf("job %zu leg %zu: %zu results against %zu\n", j, k, batch[j][k].size(), sequence[j][k].size());
                return bad + 1;
            }
            for (size_t i = 0; i < batch[j][k].size(); ++i) {
                const fks::SimulationResult &a = batch[j][k][i], &b = sequence[j][k][i];
                const bool same = a.result_config.size() == b.result_config.size() &&
                                  std::memcmp(a.result_config.data(), b.result_config.data(), a.result_config.size() * sizeof(double)) == 0 &&
                                  a.target_config == b.target_config && a.did_contact == b.did_contact &&
                                  a.outcome_is_valid == b.outcome_is_valid && a.microsteps == b.microsteps &&
                                  a.resolver_iterations == b.resolver_iterations && a.error_flags == b.error_flags;
                if (!same) {
                    if (bad < 8)
                        std::printf("job %zu leg %zu particle %zu: (%a %a %a) contact %d micro %u against (%a %a %a) contact %d micro %u\n", j,
                                    k, i, a.result_config[0], a.result_config[1], a.result_config[2], a.did_contact ? 1 : 0, a.microsteps,
                                    b.result_config[0], b.result_config[1], b.result_config[2], b.did_contact ? 1 : 0, b.microsteps);
                    ++bad;
                }
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
    const double frequency = 25.0; /* 50 controller steps */
    const uint64_t seed = 20240611;
    const size_t n = 48;
    int status = 0;
    try {
        const std::vector<int32_t> devices = test_devices();
        auto jobs_sim = fks::MakeSE2Simulator(env, params, frequency, seed, 0, devices);
        auto plain_sim = fks::MakeSE2Simulator(env, params, frequency, seed, 0, devices);
        if (const char* e = std::getenv("FKS_TEST_SHARD")) {
            if (e[0]) {
                jobs_sim->SetShardThreshold(std::strtoull(e, nullptr, 10));
                plain_sim->SetShardThreshold(std::strtoull(e, nullptr, 10));
            }
        }
        std::vector<fks::Configuration> starts;
        for (size_t i = 0; i < n; ++i)
            starts.push_back({0.6 + 0.01 * std::sin(0.7 * (double)i), 0.6 + 0.01 * std::cos(0.3 * (double)i), 0.05 * (double)(i % 7)});
        std::vector<fks::SimulationPathJob> jobs(4);
        /* the planner's edge: forward across the middle box, then back to each particle's own start */
        jobs[0].start_positions = starts;
        jobs[0].waypoints = {std::vector<fks::Configuration>(n, fks::Configuration{3.4, 3.4, 1.0}), starts};
        jobs[0].allow_contacts = true;
        /* a few particles toward the corner past the second box, ending at the first contact */
        jobs[1].start_positions.assign(starts.begin(), starts.begin() + 5);
        jobs[1].waypoints = {{{0.6, 3.4, -1.0}}};
        jobs[1].allow_contacts = false;
        /* an empty job keeps its two call indices */
        jobs[2].waypoints = {{{1.0, 1.0, 0.0}}, {{2.0, 1.0, 0.0}}};
        jobs[2].allow_contacts = true;
        /* three legs, a waypoint of its own for every particle on each */
        jobs[3].start_positions = starts;
        jobs[3].waypoints.assign(3, std::vector<fks::Configuration>(n));
        for (size_t k = 0; k < 3; ++k)
            for (size_t i = 0; i < n; ++i)
                jobs[3].waypoints[k][i] = {0.5 + 3.0 * std::fabs(std::sin(1.3 * (double)i + (double)k)),
                                           0.5 + 3.0 * std::fabs(std::cos(0.9 * (double)i + 2.0 * (double)k)),
                                           -3.0 + 0.125 * (double)((i * 7 + 11 * k) % 48)};
        jobs[3].allow_contacts = true;

        /* both simulators stand at the same call index: neither has made a call */
        const auto batch = jobs_sim->ForwardSimulateRobotsJobsAlongPaths(robot, jobs);
        std::fprintf(stderr, "path jobs: devices %zu sharded %d over %d\n", jobs_sim->Devices().size(),
                     jobs_sim->LastBatchSharded() ? 1 : 0, jobs_sim->LastBatchDevices());
        std::vector<PathResults> sequence;
        for (const fks::SimulationPathJob& job : jobs)
            sequence.push_back(plain_sim->ForwardSimulateRobotsAlongPath(robot, job.start_positions, job.waypoints, job.allow_contacts));
        int bad = differences(batch, sequence);
        size_t contacts = 0, moved = 0;
        for (const auto& job : sequence)
            for (size_t k = 0; k < job.size(); ++k)
                for (size_t i = 0; i < job[k].size(); ++i) {
                    contacts += job[k][i].did_contact ? 1 : 0;
                    if (k > 0 && job[k][i].result_config != job[k - 1][i].result_config) ++moved;
                }
        if (jobs_sim->GetStatistics() != plain_sim->GetStatistics()) {
            std::printf("statistics differ\n");
            ++bad;
        }
        if (contacts == 0 || moved == 0) {
            std::printf("no contact or no motion after the first leg in the sequence: the scene checks nothing\n");
            ++bad;
        }
        /* the batch consumed 2 + 1 + 2 + 3 call indices: the next plain calls agree again */
        const std::vector<fks::Configuration> target = {{3.4, 3.4, 1.0}};
        const auto after_batch = jobs_sim->ForwardSimulateRobots(robot, starts, target, true);
        const auto after_sequence = plain_sim->ForwardSimulateRobots(robot, starts, target, true);
        bad += differences({PathResults{after_batch}}, {PathResults{after_sequence}});
        std::printf("%zu jobs compared, %zu contacts in the sequence, %d differences\n", jobs.size(), contacts, bad);
        status = bad ? 1 : 0;
    } catch (const fks::SimulatorError& e) {
        std::fprintf(stderr, "%s\n", e.what());
        status = e.status() == FKS_ERR_NO_DEVICE ? 3 : 1;
    }
    fks_env_free(env_handle);
    return status;
}
