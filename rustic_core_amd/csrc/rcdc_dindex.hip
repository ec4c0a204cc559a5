// rcdc_dindex (include/rcdc.h): the blob index in device memory --
// ReadIndex::has / get_id of index/binarysorted.rs:230-261 and the packer's
// dedup rule (packer.rs:304-315) for ids that are already in HBM.
//
// Entries (32-byte id, 16-byte loc) stay in the order added.  An
// open-addressing table with linear probing finds them: a slot is one 64-bit
// word, (entry << 32) | tag, the tag being id bytes 8..12, so most foreign
// slots on a probe path are passed without touching their entry's id; the
// home slot is id bytes 0..8, masked.  An all-ones word is an empty slot.
//
// Insert (one lane per entry) never waits for another lane:
//   empty slot   -> compare-and-swap the lane's word in; lost the race: look
//                   at what won;
//   same id      -> 64-bit atomic min of the lane's word (same tag, so the
//                   lower entry number stays) and +1 on the slot's count;
//   another id   -> next slot.
// A slot that holds an id holds that id for good (the min only ever replaces
// a word by one of the same id), nothing is ever removed, and the host keeps
// slots >= 2 * entries, so every probe path ends, at the latest at an empty
// slot; which entry a lane sees in a slot may change under it, which id
// never.  Lowest entry and count are sums and minima over the id's entries:
// they do not depend on the order of arrival, nor on whether the table was
// rebuilt in between.
//
// Scope: the slots a workgroup reads in the insert kernel are written by
// other workgroups, on other XCDs, in the same launch, so every slot and
// count access there is an agent-scope atomic (a plain load may be served
// from a stale L1 line).  Ids and locs are written before the launch and are
// read plainly.  The lookup kernel runs after the insert kernel has ended
// and reads the table plainly.  first_new's scratch table is written with
// the insert's rule in its first kernel and read plainly in its second.

#include "rcdc_dindex.h"

namespace {

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

struct Id {
    u32x4v lo, hi;
};

__device__ __forceinline__ Id load_id(const uint8_t *base, uint64_t i) {
    const u32x4v *p = reinterpret_cast<const u32x4v *>(base + i * 32u);
    Id r;
    r.lo = p[0];
    r.hi = p[1];
    return r;
}

__device__ __forceinline__ bool same_id(const Id &a, const Id &b) {
    const u32x4v x = (a.lo ^ b.lo) | (a.hi ^ b.hi);
    return (x.x | x.y | x.z | x.w) == 0u;
}

__device__ __forceinline__ uint64_t home_of(const Id &id) {
    return ((uint64_t)id.lo.y << 32) | id.lo.x;
}

__device__ __forceinline__ uint32_t tag_of(const Id &id) { return id.lo.z; }

#define DX_RLX __ATOMIC_RELAXED
#define DX_AGENT __HIP_MEMORY_SCOPE_AGENT

// The insert rule over `slots` (mask + 1 words) for the word `mine` of an
// entry whose id is `id`; ids of the entries already there are at `ids`.
// true: the id was not in the table before.
__device__ __forceinline__ bool dx_insert(uint64_t *slots, uint32_t *counts, uint64_t mask,
                                          const uint8_t *ids, const Id &id, uint64_t mine) {
    const uint32_t tag = (uint32_t)mine;
    uint64_t h = home_of(id) & mask;
    // every pass ends the walk or moves on one slot; at most mask + 1 passes
    for (uint64_t step = 0; step <= mask; step++) {
        uint64_t cur = __hip_atomic_load(&slots[h], DX_RLX, DX_AGENT);
        if (cur == rcdc::kDxEmpty) {
            if (__hip_atomic_compare_exchange_strong(&slots[h], &cur, mine, DX_RLX, DX_RLX,
                                                     DX_AGENT))
                return true;
            // cur: the word that got there first
        }
        if ((uint32_t)cur == tag && same_id(id, load_id(ids, cur >> 32))) {
            __hip_atomic_fetch_min(&slots[h], mine, DX_RLX, DX_AGENT);
            if (counts) __hip_atomic_fetch_add(&counts[h], 1u, DX_RLX, DX_AGENT);
            return false;
        }
        h = (h + 1u) & mask;
    }
    return false;  // not reached while slots >= 2 * entries
}

// The slot of `id` read plainly (after the kernel that wrote the table), or
// kDxEmpty; *at: the slot's number.
__device__ __forceinline__ uint64_t dx_find(const uint64_t *slots, uint64_t mask,
                                            const uint8_t *ids, const Id &id, uint64_t *at) {
    const uint32_t tag = tag_of(id);
    uint64_t h = home_of(id) & mask;
    for (uint64_t step = 0; step <= mask; step++) {
        const uint64_t cur = slots[h];
        if (cur == rcdc::kDxEmpty) break;
        if ((uint32_t)cur == tag && same_id(id, load_id(ids, cur >> 32))) {
            *at = h;
            return cur;
        }
        h = (h + 1u) & mask;
    }
    return rcdc::kDxEmpty;
}

}  // namespace

__global__ __launch_bounds__(256) void rcdc_dx_fill_locs_kernel(rcdc_dindex_loc *locs,
                                                                uint64_t first, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * rcdc::kDxBlock + threadIdx.x;
    if (i >= n) return;
    u32x4v v = {RCDC_DINDEX_NO_PACK, 0u, 0u, 0u};
    *reinterpret_cast<u32x4v *>(locs + first + i) = v;
}

__global__ __launch_bounds__(256) void rcdc_dx_insert_kernel(rcdc::DxTable t, uint64_t first,
                                                             uint64_t n,
                                                             unsigned long long *keys) {
    const uint64_t i = (uint64_t)blockIdx.x * rcdc::kDxBlock + threadIdx.x;
    bool fresh = false;
    if (i < n) {
        const uint64_t e = first + i;
        const Id id = load_id(t.ids, e);
        fresh = dx_insert(t.slots, t.counts, t.mask, t.ids, id, (e << 32) | tag_of(id));
    }
    // distinct ids: one add per wave
    const unsigned long long b = __ballot(fresh);
    if (b != 0ull && (threadIdx.x & 63u) == 0u)
        __hip_atomic_fetch_add(keys, (unsigned long long)__popcll(b), DX_RLX, DX_AGENT);
}

__global__ __launch_bounds__(256) void rcdc_dx_lookup_kernel(rcdc::DxTable t,
                                                             const uint8_t *__restrict__ q,
                                                             uint64_t n, uint32_t *hits) {
    const uint64_t i = (uint64_t)blockIdx.x * rcdc::kDxBlock + threadIdx.x;
    if (i >= n) return;
    const Id id = load_id(q, i);
    uint64_t at = 0;
    const uint64_t cur = dx_find(t.slots, t.mask, t.ids, id, &at);
    uint32_t entry = RCDC_DINDEX_MISS, count = 0;
    u32x4v loc = {0u, 0u, 0u, 0u};
    if (cur != rcdc::kDxEmpty) {
        entry = (uint32_t)(cur >> 32);
        count = 1u + t.counts[at];
        loc = *reinterpret_cast<const u32x4v *>(t.locs + entry);
    }
    uint32_t *o = hits + i * 6u;  // rcdc_dindex_hit: 6 words, 4-byte aligned
    o[0] = entry;
    o[1] = count;
    o[2] = loc.x;
    o[3] = loc.y;
    o[4] = loc.z;
    o[5] = loc.w;
}

// first_new, kernel 1: a selected id that the index lacks goes into the
// scratch table under its position in the batch; out[i] = 2 marks it.
__global__ __launch_bounds__(256) void rcdc_dx_first_new_a_kernel(
    rcdc::DxTable t, const uint8_t *__restrict__ q, uint64_t n,
    const uint8_t *__restrict__ select, uint8_t *out, uint64_t *scratch, uint64_t smask) {
    const uint64_t i = (uint64_t)blockIdx.x * rcdc::kDxBlock + threadIdx.x;
    if (i >= n) return;
    uint8_t r = 0;
    if (!select || select[i] != 0) {
        const Id id = load_id(q, i);
        uint64_t at = 0;
        if (dx_find(t.slots, t.mask, t.ids, id, &at) == rcdc::kDxEmpty) {
            (void)dx_insert(scratch, nullptr, smask, q, id, (i << 32) | tag_of(id));
            r = 2;
        }
    }
    out[i] = r;
}

// kernel 2: of the marked positions, the one the scratch slot kept (the
// lowest) is the first occurrence.
__global__ __launch_bounds__(256) void rcdc_dx_first_new_b_kernel(const uint8_t *__restrict__ q,
                                                                  uint64_t n, uint8_t *out,
                                                                  const uint64_t *scratch,
                                                                  uint64_t smask) {
    const uint64_t i = (uint64_t)blockIdx.x * rcdc::kDxBlock + threadIdx.x;
    if (i >= n || out[i] != 2) return;
    const Id id = load_id(q, i);
    uint64_t at = 0;
    const uint64_t cur = dx_find(scratch, smask, q, id, &at);
    out[i] = (cur != rcdc::kDxEmpty && (cur >> 32) == i) ? 1 : 0;
}

namespace rcdc {

static inline uint32_t dx_blocks(uint64_t n) { return (uint32_t)((n + kDxBlock - 1) / kDxBlock); }

hipError_t launch_dx_fill_locs(rcdc_dindex_loc *locs, uint64_t first, uint64_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rcdc_dx_fill_locs_kernel, dim3(dx_blocks(n)), dim3(kDxBlock), 0, st, locs,
                       first, n);
    return hipGetLastError();
}

hipError_t launch_dx_insert(DxTable t, uint64_t first, uint64_t n, unsigned long long *keys,
                            hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rcdc_dx_insert_kernel, dim3(dx_blocks(n)), dim3(kDxBlock), 0, st, t, first,
                       n, keys);
    return hipGetLastError();
}

hipError_t launch_dx_lookup(DxTable t, const uint8_t *q, uint64_t n, rcdc_dindex_hit *hits,
                            hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rcdc_dx_lookup_kernel, dim3(dx_blocks(n)), dim3(kDxBlock), 0, st, t, q, n,
                       reinterpret_cast<uint32_t *>(hits));
    return hipGetLastError();
}

hipError_t launch_dx_first_new(DxTable t, const uint8_t *q, uint64_t n, const uint8_t *select,
                               uint8_t *out, uint64_t *scratch, uint64_t smask, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rcdc_dx_first_new_a_kernel, dim3(dx_blocks(n)), dim3(kDxBlock), 0, st, t, q,
                       n, select, out, scratch, smask);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rcdc_dx_first_new_b_kernel, dim3(dx_blocks(n)), dim3(kDxBlock), 0, st, q, n,
                       out, scratch, smask);
    return hipGetLastError();
}

}  // namespace rcdc
