/*
 * The batched shape-specialised module through the C++ classes (include/
 * fast_kinematic_simulator_amd/hip_particle_contact_simulator.hpp): PrepareKernels(robot,
 * batched = true) builds it at setup, BatchedSpecializationStatus() reports it, and
 * ForwardSimulateRobotsJobsAlongPaths then runs its kernels.  The scene is the SE(2) bar among
 * three boxes of path_jobs_interface_test.cpp; the job list has the shape of the Python suite's
 * SE(2) list: six jobs of 3, 2, 1, 2, 2 and 3 legs, one of them empty, one with a single
 * particle, one with per-particle waypoints, with both values of allow_contacts.  A second
 * simulator made with the same seed and specialisation off runs the same batch on the generic
 * kernels; every result is compared bitwise, and so are the statistics.
 * Exit status 0 = identical and shaped, 1 = a difference (printed), 3 = no GPU.
 *
 *   build:  python -c "from fast_kinematic_simulator_amd.build import build_shaped_batches_test; build_shaped_batches_test()"
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fast_kinematic_simulator_amd/hip_particle_contact_simulator.hpp"

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

static int differences(const std::vector<PathResults>& shaped, const std::vector<PathResults>& generic) {
    int bad = 0;
    if (shaped.size() != generic.size()) return 1;
    for (size_t j = 0; j < shaped.size(); ++j) {
        if (shaped[j].size() != generic[j].size()) return bad + 1;
        for (size_t k = 0; k < shaped[j].size(); ++k) {
            if (shaped[j][k].size() != generic[j][k].size()) return bad + 1;
            for (size_t i = 0; i < shaped[j][k].size(); ++i) {
                const fks::SimulationResult &a = shaped[j][k][i], &b = generic[j][k][i];
                const bool same = a.result_config.size() == b.result_config.size() &&
                                  std::memcmp(a.result_config.data(), b.result_config.data(), a.result_config.size() * sizeof(double)) == 0 &&
                                  a.target_config == b.target_config && a.did_contact == b.did_contact &&
                                  a.outcome_is_valid == b.outcome_is_valid && a.microsteps == b.microsteps &&
                                  a.resolver_iterations == b.resolver_iterations && a.error_flags == b.error_flags;
                if (!same) {
                    if (bad < 8) std::printf("job %zu leg %zu particle %zu differs\n", j, k, i);
                    ++bad;
                }
            }
        }
    }
    return bad;
}

static int32_t last_kernel(fks_context* ctx) {
    fks_launch_info info{};
    fks::check(fks_get_launch_info(ctx, &info), ctx, "fks_get_launch_info");
    return info.last_kernel;
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
    const size_t n = 32;
    int status = 0;
    try {
        auto shaped_sim = fks::MakeSE2Simulator(env, params, frequency, seed, 0, std::vector<int32_t>{0});
        auto generic_sim = fks::MakeSE2Simulator(env, params, frequency, seed, 0, std::vector<int32_t>{0});
        std::vector<fks::Configuration> starts;
        for (size_t i = 0; i < n; ++i)
            starts.push_back({0.6 + 0.01 * std::sin(0.7 * (double)i), 0.6 + 0.01 * std::cos(0.3 * (double)i), 0.05 * (double)(i % 7)});
        const fks::Configuration a = {3.4, 3.4, 1.0}, b = {0.6, 3.4, -1.0}, c = {3.4, 0.6, 2.0};
        std::vector<fks::SimulationPathJob> jobs(6);
        jobs[0].start_positions = starts;
        jobs[0].waypoints = {{a}, {b}, {c}};
        jobs[0].allow_contacts = true;
        jobs[1].waypoints = {{a}, {b}}; /* an empty job keeps its two call indices */
        jobs[1].allow_contacts = true;
        jobs[2].start_positions.assign(starts.begin(), starts.begin() + 1);
        jobs[2].waypoints = {{b}};
        jobs[2].allow_contacts = false;
        jobs[3].start_positions = starts; /* a waypoint of its own for every particle on each leg */
        jobs[3].waypoints.assign(2, std::vector<fks::Configuration>(n));
        for (size_t k = 0; k < 2; ++k)
            for (size_t i = 0; i < n; ++i)
                jobs[3].waypoints[k][i] = {0.5 + 3.0 * std::fabs(std::sin(1.3 * (double)i + (double)k)),
                                           0.5 + 3.0 * std::fabs(std::cos(0.9 * (double)i + 2.0 * (double)k)),
                                           -3.0 + 0.125 * (double)((i * 7 + 11 * k) % 48)};
        jobs[3].allow_contacts = true;
        jobs[4].start_positions.assign(starts.begin(), starts.begin() + 7);
        jobs[4].waypoints = {{c}, {b}};
        jobs[4].allow_contacts = false;
        jobs[5] = jobs[0];

        int bad = 0;
        const fks::SpecializationStatus plain = shaped_sim->PrepareKernels(robot, /*batched=*/true);
        const fks::SpecializationStatus batched = shaped_sim->BatchedSpecializationStatus();
        if (!batched.active || batched.failed || batched.shape.size() < 2 || batched.shape.substr(batched.shape.size() - 2) != "-b") {
            std::printf("batched module not active: shape '%s' failed %d: %s\n", batched.shape.c_str(), batched.failed ? 1 : 0,
                        batched.message.c_str());
            ++bad;
        }
        if (!plain.active || plain.shape + "-b" != batched.shape) {
            std::printf("plain module '%s' against batched '%s'\n", plain.shape.c_str(), batched.shape.c_str());
            ++bad;
        }
        /* the mode outlives the robot the first batch sets */
        fks::check(fks_set_specialization(generic_sim->context(), FKS_SPECIALIZE_OFF), generic_sim->context(), "fks_set_specialization");

        /* both simulators stand at the same call index: neither has made a call */
        const auto shaped = shaped_sim->ForwardSimulateRobotsJobsAlongPaths(robot, jobs);
        const int32_t shaped_kind = last_kernel(shaped_sim->context());
        const auto generic = generic_sim->ForwardSimulateRobotsJobsAlongPaths(robot, jobs);
        const int32_t generic_kind = last_kernel(generic_sim->context());
        if (shaped_kind != FKS_KERNEL_SHAPED_PATH_JOBS && shaped_kind != FKS_KERNEL_SHAPED_PATH_JOBS_SMALL_BATCH) {
            std::printf("the prepared simulator ran kernel kind %d\n", shaped_kind);
            ++bad;
        }
        if (generic_kind != FKS_KERNEL_PATH_JOBS && generic_kind != FKS_KERNEL_PATH_JOBS_SMALL_BATCH) {
            std::printf("the yardstick ran kernel kind %d\n", generic_kind);
            ++bad;
        }
        if (shaped_sim->BatchedSpecializationStatus().per_device.at(0).launches != 1) {
            std::printf("the batched module counts %llu launches\n",
                        (unsigned long long)shaped_sim->BatchedSpecializationStatus().per_device.at(0).launches);
            ++bad;
        }
        bad += differences(shaped, generic);
        size_t contacts = 0, moved = 0;
        for (const auto& job : generic)
            for (size_t k = 0; k < job.size(); ++k)
                for (size_t i = 0; i < job[k].size(); ++i) {
                    contacts += job[k][i].did_contact ? 1 : 0;
                    if (k > 0 && job[k][i].result_config != job[k - 1][i].result_config) ++moved;
                }
        if (shaped_sim->GetStatistics() != generic_sim->GetStatistics()) {
            std::printf("statistics differ\n");
            ++bad;
        }
        if (contacts == 0 || moved == 0) {
            std::printf("no contact or no motion after the first leg on the generic side: the scene checks nothing\n");
            ++bad;
        }
        std::printf("%zu jobs compared, kernel kind %d against %d, %zu contacts, %d differences\n", jobs.size(), shaped_kind, generic_kind,
                    contacts, bad);
        status = bad ? 1 : 0;
    } catch (const fks::SimulatorError& e) {
        std::fprintf(stderr, "%s\n", e.what());
        status = e.status() == FKS_ERR_NO_DEVICE ? 3 : 1;
    }
    fks_env_free(env_handle);
    return status;
}
