/*
 * fks_multi.cpp — one process driving several MI355X devices through the C-ABI
 * (fks_create_multi and friends, include/fks_capi.h).
 *
 * Replaces the reference's `#pragma omp parallel for` over particles (SPCS:795)
 * at device granularity: particle i of a call belongs to the device whose contiguous,
 * balanced range holds it (fks_shard_bounds), and that device
 * simulates it with first_particle_id = the range start, so the counter RNG stream of
 * every particle is the one a single device would use and the results are
 * bit-identical for any device count.  All devices share one call
 * index per logical call.  Each device gets its inputs by its own H2D copy, runs on
 * its own stream, and copies its outcomes straight into the caller's buffers at its
 * offset — the gather of per-particle outcomes is per-device D2H into host memory,
 * which is where the planner consumes them; the statistics and call counters are
 * summed over the devices (kernel_ms is the slowest device's).  Device-resident
 * multi-process use (one rank per GPU, RCCL gather) is bench.py / sharding.py.
 *
 * Host side of a call: one std::thread per active device runs that device's whole pipeline
 * (copy of its shard into its own pinned staging buffer, H2D, kernel, D2H into pinned memory,
 * copy out to the caller), so no device's copies or host memcpys wait for another device's
 * (a pageable hipMemcpyAsync blocks its caller until the copy is done, which serialised the
 * devices' copies in device order before ABI 9).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "fks_capi.h"
#include "fks_batch.h"
#include "fks_buffers.h"

struct fks_multi_context {
    struct Device {
        int32_t device = 0;
        fks_context* ctx = nullptr;
        hipStream_t stream = nullptr;
        fks_buf::ParticleStaging stage; /* the shard in HBM */
        /* pinned host staging of the shard: inputs (starts, targets), outputs (fks_buf::HostRows) */
        fks_buf::PinnedBuffer<unsigned char> h_in, h_out;
        fks_status status = FKS_OK; /* the device thread's outcome */
        std::string error;
        fks_call_counters counters{};
    }; /* move-only, as the buffers it owns */
    std::vector<Device> devices;
    std::string last_error;
    uint64_t call_index = 0;
    int32_t width = 0;
    int32_t active = 0; /* devices the batches are sharded over (0 = all) */
    fks_call_counters last{};
};

namespace {

fks_status mfail(fks_multi_context* m, fks_status st, const std::string& msg) {
    if (m) m->last_error = msg;
    return st;
}
fks_status mctx(fks_multi_context* m, fks_status st, const fks_context* ctx, const char* where) {
    return mfail(m, st, std::string(where) + ": " + fks_status_string(st) + " (" + fks_get_last_error(ctx) + ")");
}

void free_device(fks_multi_context::Device& d) {
    (void)hipSetDevice(d.device); /* before anything is freed */
    if (d.stream) (void)hipStreamDestroy(d.stream);
    if (d.ctx) fks_destroy(d.ctx); /* selects the same device */
    d = fks_multi_context::Device(); /* the buffers go with their owners */
}

int32_t active_count(const fks_multi_context* m) {
    const int32_t n = (int32_t)m->devices.size();
    return (m->active > 0 && m->active < n) ? m->active : n;
}

/* run f(device index) on one host thread per device (inline when there is one) */
template <typename F>
void on_device_threads(int32_t ndev, F f) {
    if (ndev == 1) {
        f(0);
        return;
    }
    std::vector<std::thread> threads;
    threads.reserve((size_t)ndev);
    for (int32_t g = 0; g < ndev; ++g) threads.emplace_back(f, g);
    for (auto& t : threads) t.join();
}

#define DHIP(d, expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            (d).status = FKS_ERR_HIP;                                                              \
            (d).error = std::string(#expr) + ": " + hipGetErrorString(_e);                         \
            return;                                                                                \
        }                                                                                          \
    } while (0)
#define DCTX(d, st, what)                                                                          \
    do {                                                                                           \
        const fks_status _s = (st);                                                                \
        if (_s != FKS_OK) {                                                                        \
            (d).status = _s;                                                                       \
            (d).error = std::string(what) + ": " + fks_status_string(_s) + " (" + fks_get_last_error((d).ctx) + ")"; \
            return;                                                                                \
        }                                                                                          \
    } while (0)

/* the first failing device's error, in device order */
fks_status collect_status(fks_multi_context* m, int32_t ndev) {
    for (int32_t g = 0; g < ndev; ++g) {
        const auto& d = m->devices[(size_t)g];
        if (d.status != FKS_OK) return mfail(m, d.status, "device " + std::to_string(d.device) + ": " + d.error);
    }
    return FKS_OK;
}

}  // namespace

extern "C" {

fks_status fks_shard_bounds(uint64_t n, int32_t ndev, int32_t shard, uint64_t* begin, uint64_t* end) {
    if (ndev < 1 || shard < 0 || shard >= ndev || !begin || !end) return FKS_ERR_INVALID_ARGUMENT;
    /* balanced contiguous ranges, the first n % ndev shards one particle longer
     * (fast_kinematic_simulator_amd/sharding.py shard_bounds is the same rule) */
    const uint64_t base = n / (uint64_t)ndev, extra = n % (uint64_t)ndev, g = (uint64_t)shard;
    *begin = g * base + (g < extra ? g : extra);
    *end = *begin + base + (g < extra ? 1u : 0u);
    return FKS_OK;
}

fks_status fks_create_multi(const fks_environment* env, const fks_solver_params* params, double simulation_controller_frequency,
                            uint64_t prng_seed, int32_t debug_level, const int32_t* devices, int32_t ndev,
                            fks_multi_context** out) {
    if (!out) return FKS_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!env || !params || !devices || ndev < 1 || ndev > 64) return FKS_ERR_INVALID_ARGUMENT;
    fks_multi_context* m = new (std::nothrow) fks_multi_context();
    if (!m) return FKS_ERR_OUT_OF_MEMORY;
    for (int32_t g = 0; g < ndev; ++g) {
        fks_multi_context::Device d;
        d.device = devices[g];
        fks_status st = fks_create(env, params, simulation_controller_frequency, prng_seed, debug_level, d.device, &d.ctx);
        if (st == FKS_OK && hipSetDevice(d.device) != hipSuccess) st = FKS_ERR_HIP;
        if (st == FKS_OK && hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess) st = FKS_ERR_HIP;
        m->devices.push_back(std::move(d));
        if (st != FKS_OK) {
            fks_destroy_multi(m);
            return st;
        }
    }
    *out = m;
    return FKS_OK;
}

void fks_destroy_multi(fks_multi_context* m) {
    if (!m) return;
    for (auto& d : m->devices) free_device(d);
    delete m;
}

const char* fks_multi_get_last_error(const fks_multi_context* m) { return m ? m->last_error.c_str() : "null context"; }

int32_t fks_multi_num_devices(const fks_multi_context* m) { return m ? (int32_t)m->devices.size() : 0; }

fks_context* fks_multi_device_context(fks_multi_context* m, int32_t shard) {
    if (!m || shard < 0 || shard >= (int32_t)m->devices.size()) return nullptr;
    return m->devices[(size_t)shard].ctx;
}

fks_status fks_multi_set_robot(fks_multi_context* m, const fks_robot_desc* robot) {
    if (!m) return FKS_ERR_INVALID_ARGUMENT;
    for (auto& d : m->devices) {
        const fks_status st = fks_set_robot(d.ctx, robot);
        if (st != FKS_OK) return mctx(m, st, d.ctx, "fks_set_robot");
    }
    m->width = fks_config_width(m->devices[0].ctx);
    return FKS_OK;
}

static void sum_counters(fks_multi_context* m, int32_t ndev, std::chrono::steady_clock::time_point t0);

/* fks_multi_forward_simulate (legs == 0) and fks_multi_forward_simulate_path (legs >= 1: targets
 * holds the waypoints [legs][num_targets][W], the outputs are leg-major [legs][n]...) */
static fks_status multi_simulate(fks_multi_context* m, const double* starts, uint64_t n, const double* targets, uint64_t legs,
                                 uint64_t num_targets, int32_t allow_contacts, double* out_positions, uint8_t* out_collided,
                                 uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags) {
    if (!m) return FKS_ERR_INVALID_ARGUMENT;
    if (m->width <= 0) return mfail(m, FKS_ERR_NO_ROBOT, "fks_multi_set_robot has not been called");
    if (n > 0 && (!starts || !targets || !out_positions)) return mfail(m, FKS_ERR_INVALID_ARGUMENT, "null host buffer");
    if (n > 0 && num_targets != 1 && num_targets != n) return mfail(m, FKS_ERR_INVALID_ARGUMENT, fks_batch::kTargetsOneOrN);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t W = (size_t)m->width;
    const int32_t ndev = active_count(m);
    const bool path = legs > 0;
    const uint64_t K = path ? legs : 1; /* output slices per particle */
    const uint64_t call = m->call_index;
    m->call_index += K;
    /* one host thread per device: stage in, launch, stage out (the devices run concurrently) */
    on_device_threads(ndev, [&](int32_t g) {
        auto& d = m->devices[(size_t)g];
        d.status = FKS_OK;
        d.error.clear();
        std::memset(&d.counters, 0, sizeof(d.counters));
        uint64_t lo = 0, hi = 0;
        fks_shard_bounds(n, ndev, g, &lo, &hi);
        const uint64_t k = hi - lo;
        DCTX(d, fks_set_call_index(d.ctx, call), "fks_set_call_index");
        DHIP(d, hipSetDevice(d.device));
        const uint64_t rows = k * K; /* the shard's output rows: a path's are leg-major [K][k] */
        fks_buf::ParticleStaging& sg = d.stage;
        DHIP(d, sg.reserve_rows(rows, W));
        const uint64_t nt = (num_targets == n) ? k : 1; /* per leg */
        DHIP(d, sg.reserve_targets(nt * K, W));
        if (k == 0) {
            DCTX(d, fks_get_last_call_counters(d.ctx, &d.counters), "fks_get_last_call_counters"); /* settles */
            std::memset(&d.counters, 0, sizeof(d.counters));
            return;
        }
        DHIP(d, d.h_in.reserve((k + nt * K) * W * sizeof(double)));
        DHIP(d, d.h_out.reserve(fks_buf::HostRows::bytes(rows, W)));
        double* h_starts = reinterpret_cast<double*>(d.h_in.get());
        double* h_targets = h_starts + k * W;
        std::memcpy(h_starts, starts + lo * W, k * W * sizeof(double));
        for (uint64_t leg = 0; leg < K; ++leg) /* the shard's rows of every leg's targets */
            std::memcpy(h_targets + leg * nt * W, targets + (leg * num_targets + (num_targets == n ? lo : 0)) * W,
                        nt * W * sizeof(double));
        DHIP(d, hipMemcpyAsync(sg.starts.get(), h_starts, k * W * sizeof(double), hipMemcpyHostToDevice, d.stream));
        DHIP(d, hipMemcpyAsync(sg.targets.get(), h_targets, nt * K * W * sizeof(double), hipMemcpyHostToDevice, d.stream));
        if (path)
            DCTX(d, fks_forward_simulate_path_device(d.ctx, sg.starts.get(), k, sg.targets.get(), legs, nt, lo, allow_contacts,
                                                     sg.out.get(), sg.coll.get(), sg.micro.get(), sg.res.get(), sg.err.get(), d.stream, 0),
                 "fks_forward_simulate_path_device");
        else
            DCTX(d, fks_forward_simulate_device(d.ctx, sg.starts.get(), k, sg.targets.get(), nt, lo, allow_contacts, sg.out.get(),
                                                sg.coll.get(), sg.micro.get(), sg.res.get(), sg.err.get(), d.stream, 0),
                 "fks_forward_simulate_device");
        const fks_buf::HostRows h(d.h_out.get(), rows, W);
        DHIP(d, sg.download_async(rows, W, h, d.stream));
        DHIP(d, hipStreamSynchronize(d.stream));
        for (uint64_t leg = 0; leg < K; ++leg) {
            const uint64_t src = leg * k, dst = leg * n + lo;
            std::memcpy(out_positions + dst * W, h.q + src * W, k * W * sizeof(double));
            if (out_collided) std::memcpy(out_collided + dst, h.coll + src, k);
            if (out_microsteps) std::memcpy(out_microsteps + dst, h.micro + src, k * sizeof(uint32_t));
            if (out_resolver_iterations) std::memcpy(out_resolver_iterations + dst, h.res + src, k * sizeof(uint32_t));
            if (out_error_flags) std::memcpy(out_error_flags + dst, h.err + src, k * sizeof(uint32_t));
        }
        DCTX(d, fks_get_last_call_counters(d.ctx, &d.counters), "fks_get_last_call_counters"); /* settles the launch */
    });
    const fks_status st = collect_status(m, ndev);
    if (st != FKS_OK) return st;
    sum_counters(m, ndev, t0);
    return FKS_OK;
}

/* the call's counters: the devices' sums, the longest device's kernel time */
static void sum_counters(fks_multi_context* m, int32_t ndev, std::chrono::steady_clock::time_point t0) {
    std::memset(&m->last, 0, sizeof(m->last));
    for (int32_t g = 0; g < ndev; ++g) {
        const fks_call_counters& c = m->devices[(size_t)g].counters;
        m->last.particles += c.particles;
        m->last.controller_steps += c.controller_steps;
        m->last.microsteps += c.microsteps;
        m->last.resolver_iterations += c.resolver_iterations;
        m->last.sdf_bytes += c.sdf_bytes;
        m->last.error_particles += c.error_particles;
        m->last.least_squares_rows += c.least_squares_rows;
        m->last.self_collision_checks += c.self_collision_checks;
        m->last.self_corrected_points += c.self_corrected_points;
        m->last.kernel_ms = std::max(m->last.kernel_ms, c.kernel_ms);
    }
    m->last.calls = 1;
    m->last.call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

fks_status fks_multi_forward_simulate(fks_multi_context* m, const double* starts, uint64_t n, const double* targets,
                                      uint64_t num_targets, int32_t allow_contacts, double* out_positions, uint8_t* out_collided,
                                      uint32_t* out_microsteps, uint32_t* out_resolver_iterations, uint32_t* out_error_flags) {
    return multi_simulate(m, starts, n, targets, 0, num_targets, allow_contacts, out_positions, out_collided, out_microsteps,
                          out_resolver_iterations, out_error_flags);
}

fks_status fks_multi_forward_simulate_path(fks_multi_context* m, const double* starts, uint64_t n, const double* waypoints,
                                           uint64_t num_legs, uint64_t num_targets, int32_t allow_contacts, double* out_positions,
                                           uint8_t* out_collided, uint32_t* out_microsteps, uint32_t* out_resolver_iterations,
                                           uint32_t* out_error_flags) {
    if (!m) return FKS_ERR_INVALID_ARGUMENT;
    if (num_legs == 0) return mfail(m, FKS_ERR_INVALID_ARGUMENT, "a path needs at least one leg");
    return multi_simulate(m, starts, n, waypoints, num_legs, num_targets, allow_contacts, out_positions, out_collided,
                          out_microsteps, out_resolver_iterations, out_error_flags);
}

/* fks_multi_forward_simulate_jobs and _path_jobs: the batch in its normal form (fks_batch.h: a job
 * is a path job of one leg), the concatenated particle range cut into one shard per device, and
 * each shard run through the entry's own device call, so it runs the kernels of its own form */
static fks_status multi_batch(fks_multi_context* m, fks_batch::Batch& b) {
    if (!m) return FKS_ERR_INVALID_ARGUMENT;
    if (m->width <= 0) return mfail(m, FKS_ERR_NO_ROBOT, "fks_multi_set_robot has not been called");
    std::string why;
    const fks_status refused = fks_batch::check_arguments(&b, /*individual_jacobians: the devices' contexts refuse*/ false, &why);
    if (refused != FKS_OK) return mfail(m, refused, why);
    const fks_path_job* jobs = b.jobs();
    const uint64_t num_jobs = b.num_jobs;
    std::vector<uint64_t> first((size_t)num_jobs + 1, 0); /* the jobs' first particles in the concatenated range */
    for (uint64_t j = 0; j < num_jobs; ++j) first[j + 1] = first[j] + jobs[j].n;
    const uint64_t N = b.total;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t W = (size_t)m->width;
    const int32_t ndev = active_count(m);
    const uint64_t call = m->call_index;
    /* one host thread per device: stage in, launch, stage out (the devices run concurrently) */
    on_device_threads(ndev, [&](int32_t g) {
        auto& d = m->devices[(size_t)g];
        d.status = FKS_OK;
        d.error.clear();
        std::memset(&d.counters, 0, sizeof(d.counters));
        uint64_t lo = 0, hi = 0;
        fks_shard_bounds(N, ndev, g, &lo, &hi);
        const uint64_t k = hi - lo;
        /* the device's jobs: of every job the shard meets its rows [a, b) of every leg, every
         * other job empty with its legs kept (the same call indices on every device) */
        std::vector<fks_path_job> dev((size_t)num_jobs);
        std::vector<uint64_t> row0((size_t)num_jobs, 0); /* the sub-range's first row within its job */
        uint64_t nt = 0, rows = 0; /* the shard's waypoint rows and leg-major output rows */
        for (uint64_t j = 0; j < num_jobs; ++j) {
            const uint64_t a = std::max(first[j], lo), e = std::min(first[j + 1], hi);
            fks_path_job& s = dev[j];
            std::memset(&s, 0, sizeof(s));
            s.num_legs = jobs[j].num_legs;
            s.num_targets = 1; /* an empty job: 1 is always accepted */
            if (a >= e) continue;
            row0[j] = a - first[j];
            s.n = e - a;
            s.num_targets = (jobs[j].num_targets == jobs[j].n && jobs[j].n != 1) ? s.n : 1;
            s.first_particle_id = jobs[j].first_particle_id + row0[j];
            s.allow_contacts = jobs[j].allow_contacts;
            nt += s.num_targets * s.num_legs;
            rows += s.n * s.num_legs;
        }
        DCTX(d, fks_set_call_index(d.ctx, call), "fks_set_call_index");
        DHIP(d, hipSetDevice(d.device));
        fks_buf::ParticleStaging& sg = d.stage;
        DHIP(d, sg.reserve_rows(rows, W));
        DHIP(d, sg.reserve_targets(nt, W));
        DHIP(d, d.h_in.reserve((k + nt) * W * sizeof(double)));
        DHIP(d, d.h_out.reserve(fks_buf::HostRows::bytes(rows, W)));
        double* h_starts = reinterpret_cast<double*>(d.h_in.get());
        double* h_targets = h_starts + k * W;
        uint64_t at = 0, tat = 0, oat = 0;
        for (uint64_t j = 0; j < num_jobs; ++j) {
            fks_path_job& s = dev[j];
            if (s.n == 0) continue;
            const fks_path_job& job = jobs[j];
            std::memcpy(h_starts + at * W, job.starts + row0[j] * W, s.n * W * sizeof(double));
            const uint64_t from = (s.num_targets == 1 && job.num_targets == 1) ? 0 : row0[j];
            for (uint64_t leg = 0; leg < s.num_legs; ++leg) /* the sub-range's rows of every leg's waypoints */
                std::memcpy(h_targets + (tat + leg * s.num_targets) * W, job.waypoints + (leg * job.num_targets + from) * W,
                            s.num_targets * W * sizeof(double));
            s.starts = sg.starts.get() + at * W;
            s.waypoints = sg.targets.get() + tat * W;
            sg.stage_outputs(&s, oat, W);
            at += s.n;
            tat += s.num_targets * s.num_legs;
            oat += s.n * s.num_legs;
        }
        if (k > 0) {
            DHIP(d, hipMemcpyAsync(sg.starts.get(), h_starts, k * W * sizeof(double), hipMemcpyHostToDevice, d.stream));
            DHIP(d, hipMemcpyAsync(sg.targets.get(), h_targets, nt * W * sizeof(double), hipMemcpyHostToDevice, d.stream));
        }
        if (b.form == fks_batch::JOBS) {
            std::vector<fks_job> as_jobs((size_t)num_jobs);
            for (uint64_t j = 0; j < num_jobs; ++j) as_jobs[j] = fks_batch::as_job(dev[j]);
            DCTX(d, fks_forward_simulate_jobs_device(d.ctx, as_jobs.data(), num_jobs, d.stream, 0), "fks_forward_simulate_jobs_device");
        } else {
            DCTX(d, fks_forward_simulate_path_jobs_device(d.ctx, dev.data(), num_jobs, d.stream, 0),
                 "fks_forward_simulate_path_jobs_device");
        }
        if (k == 0) {
            DCTX(d, fks_get_last_call_counters(d.ctx, &d.counters), "fks_get_last_call_counters"); /* settles */
            std::memset(&d.counters, 0, sizeof(d.counters));
            return;
        }
        const fks_buf::HostRows h(d.h_out.get(), rows, W);
        DHIP(d, sg.download_async(rows, W, h, d.stream));
        DHIP(d, hipStreamSynchronize(d.stream));
        oat = 0;
        for (uint64_t j = 0; j < num_jobs; ++j) {
            const fks_path_job& s = dev[j];
            const fks_path_job& job = jobs[j];
            if (s.n == 0) continue;
            for (uint64_t leg = 0; leg < s.num_legs; ++leg) {
                const uint64_t src = oat + leg * s.n, dst = leg * job.n + row0[j];
                std::memcpy(job.out_positions + dst * W, h.q + src * W, s.n * W * sizeof(double));
                if (job.out_collided) std::memcpy(job.out_collided + dst, h.coll + src, s.n);
                if (job.out_microsteps) std::memcpy(job.out_microsteps + dst, h.micro + src, s.n * sizeof(uint32_t));
                if (job.out_resolver_iterations) std::memcpy(job.out_resolver_iterations + dst, h.res + src, s.n * sizeof(uint32_t));
                if (job.out_error_flags) std::memcpy(job.out_error_flags + dst, h.err + src, s.n * sizeof(uint32_t));
            }
            oat += s.n * s.num_legs;
        }
        DCTX(d, fks_get_last_call_counters(d.ctx, &d.counters), "fks_get_last_call_counters"); /* settles the launch */
    });
    const fks_status st = collect_status(m, ndev);
    if (st != FKS_OK) return st; /* a refusal by the devices' contexts leaves the call index where it was */
    m->call_index = call + b.legs;  /* a job batch's jobs, a path-job batch's sum of legs */
    sum_counters(m, ndev, t0);
    return FKS_OK;
}

fks_status fks_multi_forward_simulate_jobs(fks_multi_context* m, const fks_job* jobs, uint64_t num_jobs) {
    fks_batch::Batch b;
    fks_batch::from_jobs(&b, jobs, num_jobs);
    return multi_batch(m, b);
}

fks_status fks_multi_forward_simulate_path_jobs(fks_multi_context* m, const fks_path_job* jobs, uint64_t num_jobs) {
    fks_batch::Batch b;
    fks_batch::from_path_jobs(&b, jobs, num_jobs);
    return multi_batch(m, b);
}

fks_status fks_multi_set_active_devices(fks_multi_context* m, int32_t count) {
    if (!m || count < 0 || count > (int32_t)m->devices.size()) return FKS_ERR_INVALID_ARGUMENT;
    m->active = count;
    return FKS_OK;
}

int32_t fks_multi_active_devices(const fks_multi_context* m) { return m ? active_count(m) : 0; }

fks_status fks_multi_get_statistics(const fks_multi_context* m, fks_statistics* out) {
    if (!m || !out) return FKS_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof(*out));
    for (const auto& d : m->devices) {
        fks_statistics s;
        const fks_status st = fks_get_statistics(d.ctx, &s);
        if (st != FKS_OK) return st;
        out->successful_resolves += s.successful_resolves;
        out->unsuccessful_resolves += s.unsuccessful_resolves;
        out->free_resolves += s.free_resolves;
        out->collision_resolves += s.collision_resolves;
        out->fallback_resolves += s.fallback_resolves;
        out->unsuccessful_env_collision_resolves += s.unsuccessful_env_collision_resolves;
        out->unsuccessful_self_collision_resolves += s.unsuccessful_self_collision_resolves;
        out->recovered_unsuccessful_resolves += s.recovered_unsuccessful_resolves;
    }
    return FKS_OK;
}

fks_status fks_multi_reset_statistics(fks_multi_context* m) {
    if (!m) return FKS_ERR_INVALID_ARGUMENT;
    for (auto& d : m->devices) {
        const fks_status st = fks_reset_statistics(d.ctx);
        if (st != FKS_OK) return mctx(m, st, d.ctx, "fks_reset_statistics");
    }
    return FKS_OK;
}

fks_status fks_multi_get_last_call_counters(const fks_multi_context* m, fks_call_counters* out) {
    if (!m || !out) return FKS_ERR_INVALID_ARGUMENT;
    *out = m->last;
    return FKS_OK;
}

fks_status fks_multi_set_call_index(fks_multi_context* m, uint64_t call_index) {
    if (!m) return FKS_ERR_INVALID_ARGUMENT;
    m->call_index = call_index;
    return FKS_OK;
}

fks_status fks_multi_check_config_collision(fks_multi_context* m, const double* configs, uint64_t n, double inflation_ratio,
                                            uint8_t* out_collided, uint32_t* out_error_flags) {
    if (!m) return FKS_ERR_INVALID_ARGUMENT;
    if (m->width <= 0) return mfail(m, FKS_ERR_NO_ROBOT, "fks_multi_set_robot has not been called");
    if (n > 0 && (!configs || !out_collided)) return mfail(m, FKS_ERR_INVALID_ARGUMENT, "null host buffer");
    const size_t W = (size_t)m->width;
    const int32_t ndev = active_count(m);
    /* the configurations and flags reuse the simulation buffers (starts, collided, errors) */
    on_device_threads(ndev, [&](int32_t g) {
        auto& d = m->devices[(size_t)g];
        d.status = FKS_OK;
        d.error.clear();
        uint64_t lo = 0, hi = 0;
        fks_shard_bounds(n, ndev, g, &lo, &hi);
        const uint64_t k = hi - lo;
        DHIP(d, hipSetDevice(d.device));
        fks_buf::ParticleStaging& sg = d.stage;
        DHIP(d, sg.reserve_rows(k, W));
        if (k == 0) return;
        DHIP(d, d.h_in.reserve(k * W * sizeof(double)));
        DHIP(d, d.h_out.reserve(k * (1 + sizeof(uint32_t))));
        std::memcpy(d.h_in.get(), configs + lo * W, k * W * sizeof(double));
        DHIP(d, hipMemcpyAsync(sg.starts.get(), d.h_in.get(), k * W * sizeof(double), hipMemcpyHostToDevice, d.stream));
        DCTX(d, fks_check_config_collision_device(d.ctx, sg.starts.get(), k, inflation_ratio, sg.coll.get(), sg.err.get(), d.stream, 0),
             "fks_check_config_collision_device");
        uint32_t* h_err = reinterpret_cast<uint32_t*>(d.h_out.get());
        uint8_t* h_coll = reinterpret_cast<uint8_t*>(h_err + k);
        DHIP(d, hipMemcpyAsync(h_coll, sg.coll.get(), k, hipMemcpyDeviceToHost, d.stream));
        DHIP(d, hipMemcpyAsync(h_err, sg.err.get(), k * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
        DHIP(d, hipStreamSynchronize(d.stream));
        std::memcpy(out_collided + lo, h_coll, k);
        if (out_error_flags) std::memcpy(out_error_flags + lo, h_err, k * sizeof(uint32_t));
        fks_call_counters c;
        DCTX(d, fks_get_last_check_counters(d.ctx, &c), "fks_get_last_check_counters"); /* settles the device's check */
    });
    return collect_status(m, ndev);
}

int32_t fks_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
