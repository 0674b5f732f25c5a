/*
 * fks_buffers.h — the owners of the host code's device and pinned memory.
 *
 * A block and its size are one object: a buffer that reports a capacity holds a block of at
 * least that many elements, and a growth that fails leaves it empty with capacity 0, so the
 * next call allocates again instead of trusting a stale size.  Growth is exact and frees the old
 * block before it allocates the new one (the HBM footprint and its peak are those of the
 * requests).  The callers settle their stream before they reserve: nothing in flight reads a
 * block that is given back.
 *
 * Only the HIP runtime API: a host compiler builds this header (tests/cpp/buffers_test.cpp).
 */
#ifndef FKS_BUFFERS_H
#define FKS_BUFFERS_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

namespace fks_buf {

/* one block of HBM (hipMalloc) or of pinned host memory (hipHostMalloc), move-only, freed with
 * its owner: DeviceBuffer<T> and PinnedBuffer<T> below */
template <typename T, bool kPinned>
class Buffer {
  public:
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) adopt(std::exchange(o.p_, nullptr), std::exchange(o.cap_, 0));
        return *this;
    }
    ~Buffer() { reset(); }

    T* get() const { return p_; }
    size_t capacity() const { return cap_; } /* in elements; 0 when empty */

    /* a block of at least `count` elements (of one element for count == 0): the current one
     * while the request fits it, otherwise a new one of exactly that size, allocated after the
     * old one is freed; its contents are not kept */
    hipError_t reserve(size_t count) {
        if (p_ && count <= cap_) return hipSuccess;
        reset();
        const size_t n = count > 0 ? count : 1;
        void* p = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&p, n * sizeof(T), 0) : hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        cap_ = n;
        return hipSuccess;
    }
    void reset() {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    /* takes over a block of `count` elements allocated elsewhere (null: none) */
    void adopt(T* p, size_t count) {
        reset();
        p_ = p;
        cap_ = p ? count : 0;
    }

  private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <typename T>
using DeviceBuffer = Buffer<T, false>;
template <typename T>
using PinnedBuffer = Buffer<T, true>;

/* a device block and its pinned staging copy, reserved together */
template <typename T>
class MirroredBuffer {
  public:
    T* dev() const { return dev_.get(); }
    T* host() const { return host_.get(); }
    size_t capacity() const { return std::min(dev_.capacity(), host_.capacity()); } /* what both halves hold */
    hipError_t reserve(size_t count) {
        if (dev_.get() && host_.get() && count <= capacity()) return hipSuccess;
        reset();
        hipError_t e = dev_.reserve(count);
        if (e == hipSuccess) e = host_.reserve(count);
        if (e != hipSuccess) reset();
        return e;
    }
    void reset() {
        host_.reset();
        dev_.reset();
    }

  private:
    DeviceBuffer<T> dev_;
    PinnedBuffer<T> host_;
};

/* the packed host block of a call's outputs over `rows` rows of width W: positions, microsteps,
 * resolver iterations, error bits, collided bytes */
struct HostRows {
    double* q;
    uint32_t* micro;
    uint32_t* res;
    uint32_t* err;
    uint8_t* coll;
    static size_t bytes(size_t rows, size_t W) { return rows * W * sizeof(double) + rows * (1 + 3 * sizeof(uint32_t)); }
    HostRows(void* block, size_t rows, size_t W)
        : q(static_cast<double*>(block)),
          micro(reinterpret_cast<uint32_t*>(q + rows * W)),
          res(micro + rows),
          err(res + rows),
          coll(reinterpret_cast<uint8_t*>(err + rows)) {}
};

/* the device staging of the host entries: a call's particles (starts, which a batch also fills
 * with its waypoints), its targets and its five per-row outputs */
struct ParticleStaging {
    DeviceBuffer<double> starts, targets, out;
    DeviceBuffer<uint8_t> coll;
    DeviceBuffer<uint32_t> micro, res, err;

    /* the six per-row buffers for `rows` rows of width W */
    hipError_t reserve_rows(size_t rows, size_t W) {
        hipError_t e = starts.reserve(rows * W);
        if (e == hipSuccess) e = out.reserve(rows * W);
        if (e == hipSuccess) e = coll.reserve(rows);
        if (e == hipSuccess) e = micro.reserve(rows);
        if (e == hipSuccess) e = res.reserve(rows);
        if (e == hipSuccess) e = err.reserve(rows);
        return e;
    }
    hipError_t reserve_targets(size_t count, size_t W) { return targets.reserve(count * W); }

    /* points a job's (fks_job, fks_path_job) five outputs at the staging rows from `first_row` on */
    template <typename Job>
    void stage_outputs(Job* job, size_t first_row, size_t W) const {
        job->out_positions = out.get() + first_row * W;
        job->out_collided = coll.get() + first_row;
        job->out_microsteps = micro.get() + first_row;
        job->out_resolver_iterations = res.get() + first_row;
        job->out_error_flags = err.get() + first_row;
    }

    /* `rows` rows of the outputs to the caller's arrays, one blocking copy each (null: skipped) */
    hipError_t download(size_t rows, size_t W, double* q, uint8_t* collided, uint32_t* microsteps, uint32_t* resolver,
                        uint32_t* errors) const {
        hipError_t e = hipSuccess;
        if (q) e = hipMemcpy(q, out.get(), rows * W * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess && collided) e = hipMemcpy(collided, coll.get(), rows, hipMemcpyDeviceToHost);
        if (e == hipSuccess && microsteps) e = hipMemcpy(microsteps, micro.get(), rows * sizeof(uint32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess && resolver) e = hipMemcpy(resolver, res.get(), rows * sizeof(uint32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess && errors) e = hipMemcpy(errors, err.get(), rows * sizeof(uint32_t), hipMemcpyDeviceToHost);
        return e;
    }
    /* ... or to a pinned block on `stream`, in the block's order (the caller synchronises) */
    hipError_t download_async(size_t rows, size_t W, const HostRows& h, hipStream_t stream) const {
        hipError_t e = hipMemcpyAsync(h.q, out.get(), rows * W * sizeof(double), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h.micro, micro.get(), rows * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h.res, res.get(), rows * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h.err, err.get(), rows * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h.coll, coll.get(), rows, hipMemcpyDeviceToHost, stream);
        return e;
    }
};

}  // namespace fks_buf

#endif
