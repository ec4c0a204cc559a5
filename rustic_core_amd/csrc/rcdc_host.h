// rcdc_host.h -- what the host halves of the library share: the entry points
// rcdc_runtime.cpp exports to the other units, the device guard, the error
// helpers, the owning buffers (DevBuf, PinnedBuf), and the parsers' per-call
// Scratch and tile table.  Host code only (rcdc_host_sha.cpp is built without
// HIP and does not include it).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/rcdc.h"

namespace rcdc {

// ---- exported by rcdc_runtime.cpp ------------------------------------------
int ctx_device(const rcdc_ctx *ctx);
uint64_t ctx_min_size(const rcdc_ctx *ctx);
uint64_t ctx_max_size(const rcdc_ctx *ctx);
// sets the calling thread's rcdc_last_error text and returns st
rcdc_status set_error(rcdc_status st, const char *msg);
// Rebuild `pl` (created by rcdc_plan_create, its last run waited for) for a
// new batch layout, reusing its device buffers; uploads on `up`.
rcdc_status plan_relayout(rcdc_plan *pl, const uint64_t *offs, const uint64_t *lens, uint32_t n,
                          uint64_t arena_len, hipStream_t up);

// ---- exported by rcdc_host_sha.cpp (SHA-256 on the CPU) --------------------
bool host_sha_supported();
bool host_sha_ni();
void host_sha256_many(const uint8_t *const *ptrs, const uint64_t *lens, uint32_t n,
                      uint8_t *digests);
void host_sha256_one(const uint8_t *p, uint64_t len, uint8_t out[32]);
void host_sha256_ni_many(const uint8_t *const *ptrs, const uint64_t *lens, uint32_t n,
                         uint8_t *digests, int ways);

// Makes `dev` the calling thread's current device for a scope.
struct DeviceGuard {
    int prev = 0;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(dev);
    }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

inline rcdc_status hip_fail(const char *what, hipError_t e) {
    return set_error(RCDC_ERR_INTERNAL,
                     (std::string(what) + " failed: " + hipGetErrorString(e)).c_str());
}

#define HIP_TRY(expr)                                            \
    do {                                                         \
        hipError_t e_ = (expr);                                  \
        if (e_ != hipSuccess) return rcdc::hip_fail(#expr, e_);  \
    } while (0)

inline rcdc_status invalid(const char *msg) { return set_error(RCDC_ERR_INVALID_INPUT, msg); }

// The device allocations of one call, freed when it returns.
struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <class T>
    hipError_t get(T **out, uint64_t n) {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, (n ? n : 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(p);
        *out = static_cast<T *>(p);
        return e;
    }
};

// The tile table of the parsers: the texts refs[0, n) ({off, len}) of the
// arena at d_arena are cut into tiles of tile_bytes that count from the
// 16-byte boundary at or before a text's first byte; tile_first[r] is the
// first tile of ref r and tile_first[n] = n_tiles.  within(len), called once
// per ref in order, adds what else the caller counts and returns whether that
// is still below its limit.  Returns the first check that failed; the message
// is the caller's.
// TooMany: 2^32 - 1 tiles or more, or within() said that its own count is at
// the caller's limit; the callers give one message for both.
enum class TileTable { Ok, RefOutside, ArenaNull, TooMany };
template <class Ref, class Within>
TileTable tile_table(const Ref *refs, uint32_t n, uint64_t arena_len, const void *d_arena,
                     uint32_t tile_bytes, std::vector<uint32_t> &tile_first, uint64_t &n_tiles,
                     Within within) {
    tile_first.assign(n + 1ull, 0u);
    n_tiles = 0;
    const uint64_t mis = (uint64_t)(uintptr_t)d_arena & 15u;
    for (uint32_t i = 0; i < n; i++) {
        const Ref r = refs[i];
        if (r.off > arena_len || r.len > arena_len - r.off) return TileTable::RefOutside;
        if (r.len && !d_arena) return TileTable::ArenaNull;
        const bool ok = within(r.len);
        tile_first[i] = (uint32_t)n_tiles;
        if (r.len) {
            const uint64_t v0 = (r.off + mis) & ~15ull;
            n_tiles += (r.off + mis + r.len - v0 + tile_bytes - 1) / tile_bytes;
        }
        if (n_tiles >= 0xFFFFFFFFull || !ok) return TileTable::TooMany;
    }
    tile_first[n] = (uint32_t)n_tiles;
    return TileTable::Ok;
}

// A device array that only grows, owned by the object that holds it.  Freed
// by release() or the destructor: the owner makes its device current and
// synchronises its streams before either runs.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    uint64_t capacity() const { return cap_; }  // elements

    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }

    // At least `need` elements; the contents are lost when it grows.  Grows
    // with 25 % headroom: a reallocation's hipFree synchronises the whole
    // device (every lane of every thread), so slowly varying sizes (stream
    // passes of batch + tail bytes) must not reallocate each time.
    // exact: to `need` elements and no more (prune's per-entry arrays, sized
    // once per repository).
    rcdc_status ensure(uint64_t need, bool exact = false) {
        if (need <= cap_ && p_) return RCDC_OK;
        static const bool log = getenv("RCDC_ALLOC_LOG") != nullptr;
        if (log && p_)
            fprintf(stderr, "rcdc: regrow %llu -> %llu x %zu B (hipFree: device sync)\n",
                    (unsigned long long)cap_, (unsigned long long)need, sizeof(T));
        if (p_) HIP_TRY(hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
        // at least 64 KiB: small per-stream arrays (walk streams, piece cuts)
        // otherwise regrew from 1-2 elements when a layout first had more of
        // them, each regrow a device-wide sync inside a pipeline (r5u)
        const uint64_t n =
            exact ? std::max<uint64_t>(need, 1)
                  : std::max<uint64_t>(need + need / 4, std::max<uint64_t>(65536 / sizeof(T), 1));
        HIP_TRY(hipMalloc((void **)&p_, n * sizeof(T)));
        cap_ = n;
        return RCDC_OK;
    }

private:
    T *p_ = nullptr;
    uint64_t cap_ = 0;
};

// Page-locked host memory that only grows, owned like a DevBuf (the owner's
// device is current and its streams are idle when it is freed).
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() {
        if (p_) (void)hipHostFree(p_);
    }

    uint8_t *get() const { return p_; }

    // At least `need` bytes; the contents are lost when it grows, to `grown`
    // bytes (the caller's headroom rule, >= need).
    rcdc_status ensure(uint64_t need, uint64_t grown) {
        if (need <= cap_) return RCDC_OK;
        if (p_) HIP_TRY(hipHostFree(p_));
        p_ = nullptr;
        cap_ = 0;
        HIP_TRY(hipHostMalloc((void **)&p_, grown, hipHostMallocDefault));
        cap_ = grown;
        return RCDC_OK;
    }

private:
    uint8_t *p_ = nullptr;
    uint64_t cap_ = 0;
};

}  // namespace rcdc
