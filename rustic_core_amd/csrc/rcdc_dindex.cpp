// rcdc_dindex (include/rcdc.h): the host half of the blob index in device
// memory -- the entry arrays and the table, their growth, and the ordering
// of calls.  The kernels are in rcdc_dindex.hip.
//
// Growth: before an add launches, slots >= 2 * (size + n).  When that needs
// a larger table, the new one is cleared and every entry goes through the
// same insert kernel again, so lowest entries and counts come out as they
// would have without the growth.  The entry arrays double by allocate, copy,
// free.
//
// Ordering: add waits for the lookups queued on the index (one event per
// stream that has used it) before it touches the table, and returns after
// its own stream has drained.  first_new's scratch table is used by one
// call at a time: each call waits, on its stream, for the event of the
// previous one.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "rcdc_dindex.h"
#include "rcdc_host.h"

using namespace rcdc;

struct rcdc_dindex {
    int device = 0;
    std::mutex mu;
    uint8_t *ids = nullptr;
    rcdc_dindex_loc *locs = nullptr;
    uint64_t cap = 0;  // entries the arrays hold
    uint64_t *slots = nullptr;
    uint32_t *counts = nullptr;
    uint64_t nslots = 0;
    uint64_t size = 0, keys = 0;
    unsigned long long *d_keys = nullptr;
    uint64_t *scratch = nullptr;
    uint64_t scratch_slots = 0;
    hipEvent_t scratch_ev = nullptr;
    bool scratch_used = false;
    std::vector<std::pair<hipStream_t, hipEvent_t>> readers;  // lookups since the last add
};

namespace {

constexpr uint64_t kMinSlots = 1024, kMinEntries = 512, kMaxEntries = 0xFFFFFFFFull;
constexpr size_t kMaxReaders = 16;

uint64_t pow2_at_least(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

DxTable table_of(const rcdc_dindex *dx) {
    DxTable t;
    t.slots = dx->slots;
    t.counts = dx->counts;
    t.mask = dx->nslots - 1;
    t.ids = dx->ids;
    t.locs = dx->locs;
    return t;
}

// entry arrays for `want` entries; the entries held are copied over on st
rcdc_status grow_entries(rcdc_dindex *dx, uint64_t want, hipStream_t st) {
    if (want <= dx->cap) return RCDC_OK;
    const uint64_t cap = std::max({dx->cap * 2, pow2_at_least(want), kMinEntries});
    uint8_t *ids = nullptr;
    rcdc_dindex_loc *locs = nullptr;
    HIP_TRY(hipMalloc((void **)&ids, cap * 32));
    if (hipError_t e = hipMalloc((void **)&locs, cap * sizeof(rcdc_dindex_loc)); e != hipSuccess) {
        (void)hipFree(ids);
        return hip_fail("hipMalloc(locs)", e);
    }
    if (dx->size) {
        hipError_t e = hipMemcpyAsync(ids, dx->ids, dx->size * 32, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(locs, dx->locs, dx->size * sizeof(rcdc_dindex_loc),
                               hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(ids);
            (void)hipFree(locs);
            return hip_fail("copying the entries", e);
        }
    }
    (void)hipFree(dx->ids);
    (void)hipFree(dx->locs);
    dx->ids = ids;
    dx->locs = locs;
    dx->cap = cap;
    return RCDC_OK;
}

// a cleared table of `nslots` slots in place of the old one
rcdc_status new_table(rcdc_dindex *dx, uint64_t nslots, hipStream_t st) {
    uint64_t *slots = nullptr;
    uint32_t *counts = nullptr;
    HIP_TRY(hipMalloc((void **)&slots, nslots * 8));
    if (hipError_t e = hipMalloc((void **)&counts, nslots * 4); e != hipSuccess) {
        (void)hipFree(slots);
        return hip_fail("hipMalloc(counts)", e);
    }
    (void)hipFree(dx->slots);  // no reader is left: add waited for them
    (void)hipFree(dx->counts);
    dx->slots = slots;
    dx->counts = counts;
    dx->nslots = nslots;
    HIP_TRY(hipMemsetAsync(slots, 0xFF, nslots * 8, st));
    HIP_TRY(hipMemsetAsync(counts, 0, nslots * 4, st));
    HIP_TRY(hipMemsetAsync(dx->d_keys, 0, sizeof(unsigned long long), st));
    return RCDC_OK;
}

rcdc_status wait_readers(rcdc_dindex *dx) {
    for (auto &r : dx->readers) HIP_TRY(hipEventSynchronize(r.second));
    return RCDC_OK;
}

// the work just queued on st reads the table
rcdc_status note_reader(rcdc_dindex *dx, hipStream_t st) {
    for (auto &r : dx->readers)
        if (r.first == st) {
            HIP_TRY(hipEventRecord(r.second, st));
            return RCDC_OK;
        }
    if (dx->readers.size() >= kMaxReaders) {  // reuse the oldest once its work is done
        auto r = dx->readers.front();
        HIP_TRY(hipEventSynchronize(r.second));
        dx->readers.erase(dx->readers.begin());
        r.first = st;
        HIP_TRY(hipEventRecord(r.second, st));
        dx->readers.push_back(r);
        return RCDC_OK;
    }
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    dx->readers.emplace_back(st, ev);
    HIP_TRY(hipEventRecord(ev, st));
    return RCDC_OK;
}

void free_all(rcdc_dindex *dx) {
    (void)hipFree(dx->ids);
    (void)hipFree(dx->locs);
    (void)hipFree(dx->slots);
    (void)hipFree(dx->counts);
    (void)hipFree(dx->d_keys);
    (void)hipFree(dx->scratch);
    if (dx->scratch_ev) (void)hipEventDestroy(dx->scratch_ev);
    for (auto &r : dx->readers) (void)hipEventDestroy(r.second);
}

}  // namespace

extern "C" {

rcdc_status rcdc_dindex_create(rcdc_ctx *ctx, uint64_t reserve_entries, rcdc_dindex **out) {
    if (!ctx) return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_create: ctx is NULL");
    if (!out) return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_create: out is NULL");
    if (reserve_entries >= kMaxEntries)
        return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_create: more than 2^32 - 2 entries");
    rcdc_dindex *dx = new rcdc_dindex;
    dx->device = ctx_device(ctx);
    DeviceGuard g(dx->device);
    rcdc_status rs = RCDC_OK;
    if (hipError_t e = hipMalloc((void **)&dx->d_keys, sizeof(unsigned long long)); e != hipSuccess)
        rs = hip_fail("hipMalloc(keys)", e);
    if (!rs)
        if (hipError_t e = hipEventCreateWithFlags(&dx->scratch_ev, hipEventDisableTiming);
            e != hipSuccess)
            rs = hip_fail("hipEventCreate", e);
    if (!rs) rs = grow_entries(dx, std::max<uint64_t>(reserve_entries, 1), nullptr);
    if (!rs) rs = new_table(dx, std::max(pow2_at_least(2 * reserve_entries), kMinSlots), nullptr);
    if (!rs)
        if (hipError_t e = hipStreamSynchronize(nullptr); e != hipSuccess)
            rs = hip_fail("hipStreamSynchronize", e);
    if (rs) {
        free_all(dx);
        delete dx;
        return rs;
    }
    *out = dx;
    return RCDC_OK;
}

void rcdc_dindex_destroy(rcdc_dindex *dx) {
    if (!dx) return;
    {
        DeviceGuard g(dx->device);
        for (auto &r : dx->readers) (void)hipEventSynchronize(r.second);
        if (dx->scratch_used) (void)hipEventSynchronize(dx->scratch_ev);
        free_all(dx);
    }
    delete dx;
}

uint64_t rcdc_dindex_size(const rcdc_dindex *dx) { return dx ? dx->size : 0; }
uint64_t rcdc_dindex_keys(const rcdc_dindex *dx) { return dx ? dx->keys : 0; }

rcdc_status rcdc_dindex_add(rcdc_dindex *dx, const void *ids, const rcdc_dindex_loc *locs,
                            uint64_t n, uint32_t flags, void *hip_stream) {
    if (!dx) return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_add: index is NULL");
    if (flags & ~RCDC_DINDEX_DEVICE_PTRS)
        return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_add: unknown flag bits");
    if (n && !ids) return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_add: ids is NULL");
    std::lock_guard<std::mutex> lk(dx->mu);
    if (n >= kMaxEntries || dx->size + n >= kMaxEntries)
        return set_error(RCDC_ERR_INVALID_INPUT,
                         "rcdc_dindex_add: the index would pass 2^32 - 2 entries");
    if (n == 0) return RCDC_OK;
    DeviceGuard g(dx->device);
    hipStream_t st = (hipStream_t)hip_stream;
    rcdc_status rs;
    if ((rs = wait_readers(dx))) return rs;
    const uint64_t total = dx->size + n;
    if ((rs = grow_entries(dx, total, st))) return rs;
    const hipMemcpyKind kind =
        (flags & RCDC_DINDEX_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpyAsync(dx->ids + dx->size * 32, ids, n * 32, kind, st));
    if (locs)
        HIP_TRY(hipMemcpyAsync(dx->locs + dx->size, locs, n * sizeof(rcdc_dindex_loc), kind, st));
    else
        HIP_TRY(launch_dx_fill_locs(dx->locs, dx->size, n, st));
    if (dx->nslots < 2 * total) {
        // every entry again, into a cleared table
        if ((rs = new_table(dx, std::max(dx->nslots * 2, pow2_at_least(2 * total)), st)))
            return rs;
        HIP_TRY(launch_dx_insert(table_of(dx), 0, total, dx->d_keys, st));
    } else {
        HIP_TRY(launch_dx_insert(table_of(dx), dx->size, n, dx->d_keys, st));
    }
    unsigned long long keys = 0;
    HIP_TRY(hipMemcpyAsync(&keys, dx->d_keys, sizeof keys, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    dx->size = total;
    dx->keys = keys;
    return RCDC_OK;
}

rcdc_status rcdc_dindex_lookup(rcdc_dindex *dx, const void *d_ids, uint64_t n,
                               rcdc_dindex_hit *d_hits, void *hip_stream) {
    if (!dx) return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_lookup: index is NULL");
    if (n && (!d_ids || !d_hits))
        return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_lookup: null array");
    if (n >= kMaxEntries)
        return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_lookup: more than 2^32 - 2 ids");
    if (((uintptr_t)d_ids & 15u) || ((uintptr_t)d_hits & 3u))
        return set_error(RCDC_ERR_INVALID_INPUT,
                         "rcdc_dindex_lookup: ids must be 16-byte and hits 4-byte aligned");
    if (n == 0) return RCDC_OK;
    std::lock_guard<std::mutex> lk(dx->mu);
    DeviceGuard g(dx->device);
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(launch_dx_lookup(table_of(dx), (const uint8_t *)d_ids, n, d_hits, st));
    return note_reader(dx, st);
}

rcdc_status rcdc_dindex_first_new(rcdc_dindex *dx, const void *d_ids, uint64_t n,
                                  const uint8_t *d_select, uint8_t *d_new, void *hip_stream) {
    if (!dx) return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_first_new: index is NULL");
    if (n && (!d_ids || !d_new))
        return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_first_new: null array");
    if (n >= kMaxEntries)
        return set_error(RCDC_ERR_INVALID_INPUT, "rcdc_dindex_first_new: more than 2^32 - 2 ids");
    if ((uintptr_t)d_ids & 15u)
        return set_error(RCDC_ERR_INVALID_INPUT,
                         "rcdc_dindex_first_new: ids must be 16-byte aligned");
    if (n == 0) return RCDC_OK;
    std::lock_guard<std::mutex> lk(dx->mu);
    DeviceGuard g(dx->device);
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t need = std::max(pow2_at_least(2 * n), kMinSlots);
    if (need > dx->scratch_slots) {
        if (dx->scratch_used) HIP_TRY(hipEventSynchronize(dx->scratch_ev));
        (void)hipFree(dx->scratch);
        dx->scratch = nullptr;
        dx->scratch_slots = 0;
        HIP_TRY(hipMalloc((void **)&dx->scratch, need * 8));
        dx->scratch_slots = need;
    }
    if (dx->scratch_used) HIP_TRY(hipStreamWaitEvent(st, dx->scratch_ev, 0));
    HIP_TRY(hipMemsetAsync(dx->scratch, 0xFF, need * 8, st));
    HIP_TRY(launch_dx_first_new(table_of(dx), (const uint8_t *)d_ids, n, d_select, d_new,
                               dx->scratch, need - 1, st));
    HIP_TRY(hipEventRecord(dx->scratch_ev, st));
    dx->scratch_used = true;
    return note_reader(dx, st);
}

}  // extern "C"
