/*
 * buffers_test.cpp — the owners of device and pinned memory (csrc/fks_buffers.h) without a GPU.
 * The program defines the HIP allocation and copy calls the header uses over malloc, free and
 * memcpy, counts the live blocks of each kind and can fail the k-th allocation from now on, so a
 * growth that runs out of memory half-way is an ordinary test case.  Built with AddressSanitizer:
 * a double free, a leak or a copy past a block's exact size ends the run.  Links nothing else.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "fks_buffers.h"

using namespace fks_buf;

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                  \
        }                                                                  \
    } while (0)

/* the allocator under the header */
static int g_live_device = 0, g_live_pinned = 0; /* blocks allocated and not yet freed */
static int g_allocations = 0, g_frees = 0;
static int g_fail_in = -1; /* >= 0: that many allocations succeed, the next one fails (once) */

static hipError_t allocate(void** p, size_t bytes, int* live) {
    *p = nullptr;
    if (g_fail_in == 0) {
        g_fail_in = -1;
        return hipErrorOutOfMemory;
    }
    if (g_fail_in > 0) --g_fail_in;
    if (bytes == 0) return hipErrorInvalidValue; /* the owners never ask for nothing */
    *p = std::malloc(bytes);
    ++*live;
    ++g_allocations;
    return hipSuccess;
}
static hipError_t release(void* p, int* live) {
    if (!p) return hipErrorInvalidValue; /* the owners never free nothing */
    std::free(p);
    --*live;
    ++g_frees;
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return allocate(p, bytes, &g_live_device); }
hipError_t hipFree(void* p) { return release(p, &g_live_device); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) {
    return flags == 0 ? allocate(p, bytes, &g_live_pinned) : hipErrorInvalidValue;
}
hipError_t hipHostFree(void* p) { return release(p, &g_live_pinned); }
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
}

static int live() { return g_live_device + g_live_pinned; }

/* one of a staging's buffers, whatever its element type */
struct Member {
    const void* block;
    size_t capacity, per_row;
};

static void test_reserve() {
    {
        DeviceBuffer<double> b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        const int before = g_allocations;
        CHECK(b.reserve(4) == hipSuccess && b.capacity() == 4);
        double* p4 = b.get();
        p4[3] = 1.0; /* the whole block is the buffer's (ASan) */
        CHECK(b.reserve(2) == hipSuccess && b.get() == p4 && b.capacity() == 4);
        CHECK(b.reserve(4) == hipSuccess && b.get() == p4 && b.capacity() == 4);
        CHECK(g_allocations == before + 1);
        CHECK(b.reserve(5) == hipSuccess && b.capacity() == 5); /* exact, not geometric */
        b.get()[4] = 1.0;
        CHECK(g_allocations == before + 2 && g_live_device == 1); /* the old block went first */
        b.reset();
        CHECK(b.get() == nullptr && b.capacity() == 0 && live() == 0);
        b.reset(); /* of an empty buffer: nothing to free */
        CHECK(live() == 0);
    }
    {
        DeviceBuffer<uint32_t> b;
        CHECK(b.reserve(0) == hipSuccess && b.get() != nullptr && b.capacity() == 1);
        b.get()[0] = 7u;
    }
    {
        PinnedBuffer<unsigned char> b;
        CHECK(b.reserve(3) == hipSuccess && g_live_pinned == 1 && g_live_device == 0);
        b.get()[2] = 1;
    }
    CHECK(live() == 0);
}

static void test_failed_growth() {
    DeviceBuffer<double> b;
    CHECK(b.reserve(4) == hipSuccess);
    const int frees = g_frees;
    g_fail_in = 0;
    CHECK(b.reserve(8) == hipErrorOutOfMemory);
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(g_frees == frees + 1 && live() == 0); /* the old block freed exactly once */
    /* what fitted the old block allocates again */
    CHECK(b.reserve(3) == hipSuccess && b.get() != nullptr && b.capacity() == 3);
    b.get()[2] = 1.0;
    CHECK(live() == 1);
}

static void test_staging() {
    const size_t W = 7;
    for (int k = 0; k < 6; ++k) {
        ParticleStaging s;
        CHECK(s.reserve_rows(5, W) == hipSuccess);
        CHECK(s.reserve_targets(1, W) == hipSuccess);
        CHECK(live() == 7);
        g_fail_in = k;
        CHECK(s.reserve_rows(9, W) == hipErrorOutOfMemory);
        CHECK(g_fail_in == -1);
        /* every member is whole or empty: those before the failure hold the new rows, the one
         * that failed holds nothing and says so, those after it still hold the old rows */
        const Member now[6] = {{s.starts.get(), s.starts.capacity(), W}, {s.out.get(), s.out.capacity(), W},
                               {s.coll.get(), s.coll.capacity(), 1},     {s.micro.get(), s.micro.capacity(), 1},
                               {s.res.get(), s.res.capacity(), 1},       {s.err.get(), s.err.capacity(), 1}};
        for (int i = 0; i < 6; ++i) {
            if (i == k) CHECK(now[i].block == nullptr && now[i].capacity == 0);
            else CHECK(now[i].block != nullptr && now[i].capacity == (i < k ? 9 : 5) * now[i].per_row);
        }
        CHECK(live() == 6);
        CHECK(s.targets.get() != nullptr && s.targets.capacity() == W);
        /* the stale-capacity case: fewer rows than before the failure, a healthy allocator */
        CHECK(s.reserve_rows(3, W) == hipSuccess);
        CHECK(s.starts.get() && s.out.get() && s.coll.get() && s.micro.get() && s.res.get() && s.err.get());
        CHECK(s.starts.capacity() >= 3 * W && s.out.capacity() >= 3 * W && s.coll.capacity() >= 3 && s.micro.capacity() >= 3 &&
              s.res.capacity() >= 3 && s.err.capacity() >= 3);
        /* ... and every row of every buffer is there to be written (ASan) */
        std::memset(s.starts.get(), 0, 3 * W * sizeof(double));
        std::memset(s.out.get(), 0, 3 * W * sizeof(double));
        std::memset(s.coll.get(), 0, 3);
        std::memset(s.micro.get(), 0, 3 * sizeof(uint32_t));
        std::memset(s.res.get(), 0, 3 * sizeof(uint32_t));
        std::memset(s.err.get(), 0, 3 * sizeof(uint32_t));
        CHECK(live() == 7);
    }
    CHECK(live() == 0);
    /* a wider configuration grows the two position buffers alone */
    ParticleStaging s;
    CHECK(s.reserve_rows(4, 3) == hipSuccess);
    const uint8_t* coll = s.coll.get();
    CHECK(s.reserve_rows(4, 12) == hipSuccess);
    CHECK(s.starts.capacity() == 48 && s.out.capacity() == 48 && s.coll.get() == coll && s.coll.capacity() == 4);
}

struct Job {
    double* out_positions;
    uint8_t* out_collided;
    uint32_t *out_microsteps, *out_resolver_iterations, *out_error_flags;
};

static void test_download() {
    const size_t W = 7, rows = 3;
    ParticleStaging s;
    CHECK(s.reserve_rows(rows, W) == hipSuccess);
    Job job;
    s.stage_outputs(&job, 2, W);
    CHECK(job.out_positions == s.out.get() + 2 * W && job.out_collided == s.coll.get() + 2 && job.out_microsteps == s.micro.get() + 2 &&
          job.out_resolver_iterations == s.res.get() + 2 && job.out_error_flags == s.err.get() + 2);
    for (size_t i = 0; i < rows * W; ++i) s.out.get()[i] = 1.0 + (double)i;
    for (size_t i = 0; i < rows; ++i) {
        s.coll.get()[i] = (uint8_t)(10 + i);
        s.micro.get()[i] = (uint32_t)(20 + i);
        s.res.get()[i] = (uint32_t)(30 + i);
        s.err.get()[i] = (uint32_t)(40 + i);
    }
    /* blocking, to separate arrays of the exact size; the optional ones may be absent */
    std::vector<double> q(rows * W);
    std::vector<uint8_t> coll(rows);
    std::vector<uint32_t> micro(rows), res(rows), err(rows);
    CHECK(s.download(rows, W, q.data(), coll.data(), micro.data(), res.data(), err.data()) == hipSuccess);
    CHECK(q[0] == 1.0 && q[rows * W - 1] == (double)(rows * W) && coll[2] == 12 && micro[2] == 22 && res[2] == 32 && err[2] == 42);
    std::vector<uint32_t> err2(2, 0u);
    CHECK(s.download(2, W, nullptr, nullptr, nullptr, nullptr, err2.data()) == hipSuccess);
    CHECK(err2[0] == 40 && err2[1] == 41);
    /* on a stream, into one packed block */
    PinnedBuffer<unsigned char> block;
    CHECK(block.reserve(HostRows::bytes(rows, W)) == hipSuccess);
    const HostRows h(block.get(), rows, W);
    CHECK(s.download_async(rows, W, h, nullptr) == hipSuccess);
    CHECK(h.q[rows * W - 1] == (double)(rows * W) && h.micro[0] == 20 && h.res[1] == 31 && h.err[2] == 42 && h.coll[2] == 12);
}

static void test_mirrored() {
    MirroredBuffer<uint64_t> m;
    CHECK(m.capacity() == 0 && m.dev() == nullptr && m.host() == nullptr);
    CHECK(m.reserve(4) == hipSuccess && m.capacity() == 4 && g_live_device == 1 && g_live_pinned == 1);
    const uint64_t *d4 = m.dev(), *h4 = m.host();
    CHECK(m.reserve(3) == hipSuccess && m.dev() == d4 && m.host() == h4);
    g_fail_in = 1; /* the device half succeeds, the pinned half fails */
    CHECK(m.reserve(6) == hipErrorOutOfMemory);
    CHECK(m.capacity() == 0 && m.dev() == nullptr && m.host() == nullptr && live() == 0);
    const int before = g_allocations;
    CHECK(m.reserve(2) == hipSuccess && m.capacity() == 2 && m.dev() && m.host());
    CHECK(g_allocations == before + 2 && g_live_device == 1 && g_live_pinned == 1); /* both halves again */
    m.dev()[1] = m.host()[1] = 1;
    g_fail_in = 0; /* the device half fails */
    CHECK(m.reserve(9) == hipErrorOutOfMemory && m.capacity() == 0 && live() == 0);
}

static void test_ownership() {
    const int frees = g_frees;
    {
        DeviceBuffer<double> a;
        CHECK(a.reserve(4) == hipSuccess);
        double* p = a.get();
        DeviceBuffer<double> b(std::move(a));
        CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 4);
        DeviceBuffer<double> c;
        CHECK(c.reserve(2) == hipSuccess);
        c = std::move(b); /* frees c's own block, takes b's */
        CHECK(g_frees == frees + 1 && b.get() == nullptr && b.capacity() == 0 && c.get() == p && c.capacity() == 4);
        CHECK(live() == 1);
    }
    CHECK(g_frees == frees + 2 && live() == 0); /* one free for the block that moved twice */
    {
        void* raw = nullptr;
        CHECK(hipMalloc(&raw, 6 * sizeof(float)) == hipSuccess);
        DeviceBuffer<float> b;
        CHECK(b.reserve(1) == hipSuccess);
        b.adopt(static_cast<float*>(raw), 6); /* the buffer's own block goes, the adopted one is its block now */
        CHECK(b.get() == raw && b.capacity() == 6 && live() == 1);
        b.adopt(nullptr, 6);
        CHECK(b.get() == nullptr && b.capacity() == 0 && live() == 0);
        CHECK(hipMalloc(&raw, sizeof(float)) == hipSuccess);
        b.adopt(static_cast<float*>(raw), 1);
    }
    CHECK(live() == 0);
    {
        /* owners in a vector, as the devices of a multi-device context */
        std::vector<ParticleStaging> v;
        for (int i = 0; i < 5; ++i) {
            ParticleStaging s;
            CHECK(s.reserve_rows(2, 3) == hipSuccess);
            v.push_back(std::move(s));
        }
        CHECK(live() == 30);
        v[1] = ParticleStaging();
        CHECK(live() == 24);
    }
    CHECK(live() == 0);
}

static void test_host_rows() {
    const size_t W = 7;
    for (size_t rows : {(size_t)0, (size_t)1, (size_t)3}) {
        CHECK(HostRows::bytes(rows, W) == rows * W * 8 + rows * (1 + 3 * 4));
        std::vector<unsigned char> block(HostRows::bytes(rows, W) + 1);
        const HostRows h(block.data(), rows, W);
        unsigned char* base = block.data();
        CHECK((unsigned char*)h.q == base);
        CHECK((unsigned char*)h.micro == base + rows * W * 8);
        CHECK((unsigned char*)h.res == base + rows * W * 8 + rows * 4);
        CHECK((unsigned char*)h.err == base + rows * W * 8 + rows * 8);
        CHECK((unsigned char*)h.coll == base + rows * W * 8 + rows * 12);
        CHECK(h.coll + rows == base + HostRows::bytes(rows, W));
    }
}

int main() {
    test_reserve();
    test_failed_growth();
    CHECK(live() == 0);
    test_staging();
    CHECK(live() == 0);
    test_download();
    test_mirrored();
    test_ownership();
    test_host_rows();
    CHECK(g_live_device == 0 && g_live_pinned == 0 && g_allocations == g_frees);
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("buffers test ok\n");
    return 0;
}
