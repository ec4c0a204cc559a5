// rcdc_prune (include/rcdc.h): the per-blob part of prune's plan for index
// entries in HBM -- count_used_blobs (commands/prune.rs:770-784), the
// marking of PackInfo::from_pack (:1495-1568) over all packs in processing
// order, its sums per pack, and the pick of the blobs a repack keeps.  The
// kernels first, the host half below them.
//
// The join is rcdc_dindex_lookup of every entry id against an rcdc_dindex of
// the used ids (ids without locations): hit.entry is the used number.
//
// The marking.  The sequential rule scans packs in processing order over one
// counter per used id, which starts at min(k, 255) for an id with k entries:
// a scan decrements the counter of every blob it passes, the blob that
// brings a counter to 0 makes the pack needed, and a needed pack takes
// (zeroes) every id it holds whose counter is still above 0.  So, with the
// entries of an id ordered by processing position and the first min(k, 255)
// called live:
//   (a) id x is taken by the first needed pack that holds a live entry of
//       x, and that pack exists: if none before the pack of x's last live
//       entry is needed, the counter reaches 0 there;
//   (b) pack P is needed iff some x has its last live entry in P and is not
//       taken by a pack before P;
//   (c) in a needed pack P the scan stops at the trigger: the first entry,
//       in pack order, that is the last live entry of an id P takes.  The
//       trigger's id is used at the trigger; every other id P takes is used
//       at its first entry in P.  Everything else is unused.
// An id with one entry settles at once: its pack is needed, its entry used
// and a trigger candidate.  The others go through rounds (one launch each):
// the head lane of an id walks its live entries from where it stopped; a
// NOT_NEEDED pack is passed, a NEEDED pack takes the id, the pack of the
// last live entry becomes NEEDED and takes it, an UNDECIDED pack ends the
// walk for this round.  An id taken before its last live pack takes one off
// that pack's `pending`; at 0 the pack becomes NOT_NEEDED.  Every decision
// rests on decided states only, states never change once decided, so the
// result does not depend on the interleaving; the lowest undecided pack has
// only decided packs before it, so each round decides it at least.
//
// Scope: state[], pending[], trigger[], the counts and keep's blocked[] /
// minpos[] are written and read by several workgroups in one launch and are
// touched with agent-scope atomics only.  taken[] and progress[] are written
// by the one lane that owns the id and read by it in later launches, or by
// others after the rounds have ended.  Hits, pack numbers, the sorted keys
// and the callers' arrays are written before the launch that reads them.
// No loop waits: the walk is bounded by 255, the pack loops by the pack's
// entry count.

#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rcdc.h"
#include "rcdc_host.h"

using rcdc::DeviceGuard;
using rcdc::DevBuf;
using rcdc::invalid;

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kBlock = 256;
constexpr uint32_t kLive = 255;
enum : uint32_t { UNDECIDED = 0, NEEDED = 1, NOT_NEEDED = 2 };

#define PR_RLX __ATOMIC_RELAXED
#define PR_AGENT __HIP_MEMORY_SCOPE_AGENT

// what the kernels know of the packs and entries
struct PrView {
    const rcdc_dindex_hit *hits;  // n
    const uint32_t *pack_of;      // n: processing-order pack, kNone in a gap
    const uint64_t *first;        // per pack
    const uint32_t *count;        // per pack
    const uint32_t *prefix;       // per pack: processing position of its first entry
    uint64_t n, n_packs;
};

__device__ __forceinline__ uint32_t ppos_of(const PrView &v, uint32_t p, uint64_t e) {
    return v.prefix[p] + (uint32_t)(e - v.first[p]);
}

// ids with a stride (or unaligned) -> n x 32 contiguous bytes
__global__ __launch_bounds__(256) void rcdc_pr_gather_ids_kernel(const uint8_t *__restrict__ src,
                                                                 uint64_t stride, uint64_t n,
                                                                 uint8_t *__restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;  // one byte quad each
    if (i >= n * 8) return;
    const uint64_t e = i >> 3, q = i & 7;
    const uint8_t *s = src + e * stride + q * 4;
    uint8_t *d = dst + e * 32 + q * 4;
    d[0] = s[0], d[1] = s[1], d[2] = s[2], d[3] = s[3];
}

// one workgroup per pack: the pack number of its entries
__global__ __launch_bounds__(256) void rcdc_pr_pack_of_kernel(const uint64_t *__restrict__ first,
                                                              const uint32_t *__restrict__ count,
                                                              uint64_t n, uint32_t *pack_of) {
    const uint32_t p = blockIdx.x;
    const uint64_t f = first[p];
    const uint32_t c = count[p];
    for (uint32_t i = threadIdx.x; i < c; i += kBlock)
        if (f + i < n) pack_of[f + i] = p;
}

__global__ __launch_bounds__(256) void rcdc_pr_count_kernel(PrView v, uint32_t *cnt) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= v.n || v.pack_of[e] == kNone) return;
    const uint32_t u = v.hits[e].entry;
    if (u != RCDC_DINDEX_MISS) __hip_atomic_fetch_add(&cnt[u], 1u, PR_RLX, PR_AGENT);
}

// counts out, missing ids
__global__ __launch_bounds__(256) void rcdc_pr_counts_out_kernel(const uint32_t *__restrict__ cnt,
                                                                 uint64_t m, uint8_t *d_counts,
                                                                 unsigned long long *missing,
                                                                 uint32_t *first_missing) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const uint32_t c = cnt[j];
    d_counts[j] = (uint8_t)(c > kLive ? kLive : c);
    if (c == 0) {
        __hip_atomic_fetch_add(missing, 1ull, PR_RLX, PR_AGENT);
        __hip_atomic_fetch_min(first_missing, (uint32_t)j, PR_RLX, PR_AGENT);
    }
}

// every entry: unused by default; an id with one entry is used, makes its
// pack needed and is a trigger candidate; the others are counted
__global__ __launch_bounds__(256) void rcdc_pr_singles_kernel(PrView v,
                                                              const uint32_t *__restrict__ cnt,
                                                              uint8_t *d_used, uint32_t *state,
                                                              uint32_t *trigger,
                                                              unsigned long long *ndup) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= v.n) return;
    uint8_t used = 0;
    const uint32_t p = v.pack_of[e];
    if (p != kNone) {
        const uint32_t u = v.hits[e].entry;
        if (u != RCDC_DINDEX_MISS) {
            if (cnt[u] == 1) {
                used = 1;
                __hip_atomic_store(&state[p], (uint32_t)NEEDED, PR_RLX, PR_AGENT);
                __hip_atomic_fetch_min(&trigger[p], ppos_of(v, p, e), PR_RLX, PR_AGENT);
            } else {
                __hip_atomic_fetch_add(ndup, 1ull, PR_RLX, PR_AGENT);
            }
        }
    }
    d_used[e] = used;
}

// entries of ids with two or more entries -> (used number, position) keys
__global__ __launch_bounds__(256) void rcdc_pr_compact_kernel(PrView v,
                                                              const uint32_t *__restrict__ cnt,
                                                              unsigned long long *cursor,
                                                              uint64_t cap, uint64_t *keys,
                                                              uint32_t *vals) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= v.n) return;
    const uint32_t p = v.pack_of[e];
    if (p == kNone) return;
    const uint32_t u = v.hits[e].entry;
    if (u == RCDC_DINDEX_MISS || cnt[u] < 2) return;
    const unsigned long long at = __hip_atomic_fetch_add(cursor, 1ull, PR_RLX, PR_AGENT);
    if (at >= cap) return;  // cannot happen: cap is the count of these entries
    keys[at] = ((uint64_t)u << 32) | ppos_of(v, p, e);
    vals[at] = (uint32_t)e;
}

__device__ __forceinline__ bool is_head(const uint64_t *keys, uint64_t j) {
    return j == 0 || (uint32_t)(keys[j - 1] >> 32) != (uint32_t)(keys[j] >> 32);
}

// head of each id: its last live entry's pack has one more id pending
__global__ __launch_bounds__(256) void rcdc_pr_pending_kernel(PrView v,
                                                              const uint64_t *__restrict__ keys,
                                                              const uint32_t *__restrict__ vals,
                                                              uint64_t nd,
                                                              const uint32_t *__restrict__ cnt,
                                                              uint32_t *pending) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nd || !is_head(keys, j)) return;
    const uint32_t k = cnt[(uint32_t)(keys[j] >> 32)];
    const uint64_t last = j + (k > kLive ? kLive : k) - 1;
    if (last >= nd) return;  // cannot happen: the id has k entries in the list
    __hip_atomic_fetch_add(&pending[v.pack_of[vals[last]]], 1u, PR_RLX, PR_AGENT);
}

// a pack that no single made needed and on which nothing is pending
__global__ __launch_bounds__(256) void rcdc_pr_idle_packs_kernel(uint64_t n_packs,
                                                                 const uint32_t *pending,
                                                                 uint32_t *state) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_packs) return;
    if (pending[p] == 0 && state[p] == UNDECIDED) state[p] = NOT_NEEDED;
}

// one round: the head lane of every unsettled id walks on
__global__ __launch_bounds__(256) void rcdc_pr_round_kernel(PrView v,
                                                            const uint64_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ vals,
                                                            uint64_t nd,
                                                            const uint32_t *__restrict__ cnt,
                                                            uint32_t *taken, uint32_t *progress,
                                                            uint32_t *state, uint32_t *pending,
                                                            uint32_t *trigger,
                                                            unsigned long long *unsettled) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nd || !is_head(keys, j)) return;
    const uint32_t u = (uint32_t)(keys[j] >> 32);
    if (taken[u] != kNone) return;
    const uint32_t k = cnt[u];
    const uint32_t live = k > kLive ? kLive : k;
    if (j + live > nd) return;  // cannot happen
    const uint64_t last = j + live - 1;
    const uint32_t p_last = v.pack_of[vals[last]];
    uint32_t i = progress[j];
    uint32_t took = kNone;
    for (; i < live; ++i) {
        const uint32_t p = v.pack_of[vals[j + i]];
        const uint32_t s = __hip_atomic_load(&state[p], PR_RLX, PR_AGENT);
        if (s == NEEDED) {
            took = p;
            break;
        }
        if (p == p_last) {  // every pack before it is NOT_NEEDED
            __hip_atomic_store(&state[p], (uint32_t)NEEDED, PR_RLX, PR_AGENT);
            took = p;
            break;
        }
        if (s != NOT_NEEDED) break;
    }
    if (took == kNone) {
        progress[j] = i;
        __hip_atomic_fetch_add(unsettled, 1ull, PR_RLX, PR_AGENT);
        return;
    }
    taken[u] = took;
    if (took == p_last) {
        __hip_atomic_fetch_min(&trigger[took], (uint32_t)keys[last], PR_RLX, PR_AGENT);
    } else if (__hip_atomic_fetch_sub(&pending[p_last], 1u, PR_RLX, PR_AGENT) == 1u) {
        uint32_t expect = UNDECIDED;
        __hip_atomic_compare_exchange_strong(&state[p_last], &expect, (uint32_t)NOT_NEEDED,
                                             PR_RLX, PR_RLX, PR_AGENT);
    }
}

// rule (c) for the entries of ids with two or more entries
__global__ __launch_bounds__(256) void rcdc_pr_flags_kernel(PrView v,
                                                            const uint64_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ vals,
                                                            uint64_t nd,
                                                            const uint32_t *__restrict__ taken,
                                                            const uint32_t *__restrict__ trigger,
                                                            uint8_t *d_used) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nd) return;
    const uint32_t u = (uint32_t)(keys[j] >> 32), pp = (uint32_t)keys[j];
    const uint32_t e = vals[j];
    const uint32_t p = v.pack_of[e];
    if (taken[u] != p) return;  // d_used[e] is 0 already
    const uint32_t tp = trigger[p];
    if (tp == kNone) return;  // cannot happen: a needed pack has a trigger
    const uint64_t te = v.first[p] + (tp - v.prefix[p]);
    bool used;
    if (te < v.n && v.hits[te].entry == u)
        used = pp == tp;
    else
        used = is_head(keys, j) || v.pack_of[vals[j - 1]] != p;
    if (used) d_used[e] = 1;
}

// one wave per pack: PackInfo's sums
__global__ __launch_bounds__(256) void rcdc_pr_sums_kernel(PrView v,
                                                           const uint8_t *__restrict__ d_used,
                                                           const uint8_t *__restrict__ len,
                                                           uint64_t len_stride,
                                                           const uint8_t *__restrict__ ulen,
                                                           uint64_t ulen_stride,
                                                           rcdc_prune_pack *out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (p >= v.n_packs) return;  // whole waves leave together
    const uint64_t f = v.first[p];
    const uint32_t c = v.count[p];
    unsigned long long us = 0, ns = 0;
    uint32_t ub = 0, nb = 0, raw = 0;
    for (uint32_t i = lane; i < c; i += 64) {
        const uint64_t e = f + i;
        if (e >= v.n) break;
        const uint32_t l = *reinterpret_cast<const uint32_t *>(len + e * len_stride);
        const uint32_t ul = *reinterpret_cast<const uint32_t *>(ulen + e * ulen_stride);
        if (d_used[e]) {
            us += l;
            ub += 1;
        } else {
            ns += l;
            nb += 1;
        }
        raw += ul == 0;
    }
    for (int d = 32; d > 0; d >>= 1) {
        us += __shfl_down(us, d, 64);
        ns += __shfl_down(ns, d, 64);
        ub += __shfl_down(ub, d, 64);
        nb += __shfl_down(nb, d, 64);
        raw += __shfl_down(raw, d, 64);
    }
    if (lane == 0) {
        rcdc_prune_pack r;
        r.used_size = us, r.unused_size = ns, r.used_blobs = ub, r.unused_blobs = nb;
        r.compressed = raw == 0, r.pad = 0;
        out[p] = r;
    }
}

// keep, pass 1: ids that a KEEP pack holds; lowest file position among REPACK packs
__global__ __launch_bounds__(256) void rcdc_pr_keep_a_kernel(PrView v,
                                                             const uint8_t *__restrict__ kinds,
                                                             const uint32_t *__restrict__ fprefix,
                                                             uint32_t *blocked, uint32_t *minpos) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= v.n) return;
    const uint32_t p = v.pack_of[e];
    if (p == kNone) return;
    const uint32_t u = v.hits[e].entry;
    if (u == RCDC_DINDEX_MISS) return;
    const uint32_t kind = kinds[p];
    if (kind == RCDC_PRUNE_KEEP)
        __hip_atomic_fetch_or(&blocked[u], 1u, PR_RLX, PR_AGENT);
    else if (kind == RCDC_PRUNE_REPACK)
        __hip_atomic_fetch_min(&minpos[u], fprefix[p] + (uint32_t)(e - v.first[p]), PR_RLX,
                               PR_AGENT);
}

// keep, pass 2: the compare
__global__ __launch_bounds__(256) void rcdc_pr_keep_b_kernel(PrView v,
                                                             const uint8_t *__restrict__ kinds,
                                                             const uint32_t *__restrict__ fprefix,
                                                             const uint32_t *__restrict__ blocked,
                                                             const uint32_t *__restrict__ minpos,
                                                             uint8_t *d_keep) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= v.n) return;
    uint8_t keep = 0;
    const uint32_t p = v.pack_of[e];
    if (p != kNone && kinds[p] == RCDC_PRUNE_REPACK) {
        const uint32_t u = v.hits[e].entry;
        if (u != RCDC_DINDEX_MISS && blocked[u] == 0 &&
            minpos[u] == fprefix[p] + (uint32_t)(e - v.first[p]))
            keep = 1;
    }
    d_keep[e] = keep;
}

// ---- the host half -----------------------------------------------------------

uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

constexpr uint64_t kMaxCount = 0xFFFFFFFFull;  // n, m stay below it

}  // namespace

struct rcdc_prune {
    int device = 0;
    std::mutex mu;
    rcdc_dindex *dx = nullptr;
    uint64_t m = 0;
    // entries
    bool have_entries = false;
    const uint8_t *len = nullptr, *ulen = nullptr;
    uint64_t len_stride = 0, ulen_stride = 0, n = 0, n_packs = 0;
    std::vector<rcdc_prune_range> ranges;
    // device arrays, each grown to exactly the size asked for
    DevBuf<uint8_t> ids;
    DevBuf<rcdc_dindex_hit> hits;
    DevBuf<uint32_t> pack_of, count, prefix;
    DevBuf<uint64_t> first;
    // mark
    DevBuf<uint32_t> cnt, taken, state, pending, trigger, vals_a, vals_b, progress;
    DevBuf<unsigned long long> scalars;
    DevBuf<uint64_t> keys_a, keys_b;
    DevBuf<uint8_t> sort_tmp;
    DevBuf<rcdc_prune_pack> packs_out;
    // keep
    DevBuf<uint8_t> kinds;
    DevBuf<uint32_t> fprefix, blocked, minpos;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};

    // destroyed with its device current (rcdc_prune_destroy: and synchronised)
    ~rcdc_prune() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        rcdc_dindex_destroy(dx);
    }
};

namespace {

PrView view_of(const rcdc_prune *pr) {
    PrView v;
    v.hits = pr->hits;
    v.pack_of = pr->pack_of;
    v.first = pr->first;
    v.count = pr->count;
    v.prefix = pr->prefix;
    v.n = pr->n;
    v.n_packs = pr->n_packs;
    return v;
}

}  // namespace

extern "C" {

rcdc_status rcdc_prune_create(rcdc_ctx *ctx, const void *d_used_ids, uint64_t m,
                              void *hip_stream, rcdc_prune **out) {
    if (!ctx) return invalid("rcdc_prune_create: ctx is NULL");
    if (!out) return invalid("rcdc_prune_create: out is NULL");
    if (m && !d_used_ids) return invalid("rcdc_prune_create: used ids are NULL");
    if (m >= kMaxCount) return invalid("rcdc_prune_create: more than 2^32 - 2 used ids");
    rcdc_prune *pr = new rcdc_prune;
    pr->device = rcdc::ctx_device(ctx);
    pr->m = m;
    DeviceGuard g(pr->device);
    rcdc_status rs = rcdc_dindex_create(ctx, m, &pr->dx);
    if (!rs) rs = rcdc_dindex_add(pr->dx, d_used_ids, nullptr, m, RCDC_DINDEX_DEVICE_PTRS, hip_stream);
    if (!rs && rcdc_dindex_keys(pr->dx) != m)
        rs = invalid("rcdc_prune_create: the used ids are not distinct");
    for (hipEvent_t &e : pr->ev)
        if (!rs)
            if (hipError_t he = hipEventCreate(&e); he != hipSuccess) rs = rcdc::hip_fail("hipEventCreate", he);
    if (rs) {
        delete pr;
        return rs;
    }
    *out = pr;
    return RCDC_OK;
}

void rcdc_prune_destroy(rcdc_prune *pr) {
    if (!pr) return;
    DeviceGuard g(pr->device);
    (void)hipDeviceSynchronize();
    delete pr;
}

rcdc_status rcdc_prune_set_entries(rcdc_prune *pr, const void *d_ids, uint64_t id_stride,
                                   const void *d_len, uint64_t len_stride, const void *d_ulen,
                                   uint64_t ulen_stride, uint64_t n,
                                   const rcdc_prune_range *ranges, uint64_t n_packs,
                                   void *hip_stream) {
    if (!pr) return invalid("rcdc_prune_set_entries: handle is NULL");
    if (n && (!d_ids || !d_len || !d_ulen)) return invalid("rcdc_prune_set_entries: null array");
    if (n_packs && !ranges) return invalid("rcdc_prune_set_entries: ranges are NULL");
    if (n >= kMaxCount) return invalid("rcdc_prune_set_entries: more than 2^32 - 2 entries");
    if (n_packs > 0x7FFFFFFFull) return invalid("rcdc_prune_set_entries: more than 2^31 - 1 packs");
    if (n && (id_stride < 32 || len_stride < 4 || ulen_stride < 4))
        return invalid("rcdc_prune_set_entries: a stride is smaller than its element");
    if (n && ((((uintptr_t)d_len | len_stride | (uintptr_t)d_ulen | ulen_stride) & 3u)))
        return invalid("rcdc_prune_set_entries: lengths must be 4-byte aligned");
    // ranges: inside the entries, small enough, not overlapping
    std::vector<std::pair<uint64_t, uint64_t>> sorted;
    sorted.reserve(n_packs);
    for (uint64_t p = 0; p < n_packs; ++p) {
        const rcdc_prune_range &r = ranges[p];
        if (r.count > RCDC_PRUNE_MAX_PACK_ENTRIES)
            return invalid("rcdc_prune_set_entries: a pack of 65 536 entries or more");
        if (r.first > n || r.count > n - r.first)
            return invalid("rcdc_prune_set_entries: a range past the entries");
        if (r.count) sorted.emplace_back(r.first, r.first + r.count);
    }
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < sorted.size(); ++i)
        if (sorted[i].first < sorted[i - 1].second)
            return invalid("rcdc_prune_set_entries: overlapping ranges");

    std::lock_guard<std::mutex> lk(pr->mu);
    DeviceGuard g(pr->device);
    hipStream_t st = (hipStream_t)hip_stream;
    pr->have_entries = false;
    pr->ranges.assign(ranges, ranges + n_packs);
    pr->n = n, pr->n_packs = n_packs;
    pr->len = (const uint8_t *)d_len, pr->ulen = (const uint8_t *)d_ulen;
    pr->len_stride = len_stride, pr->ulen_stride = ulen_stride;
    std::vector<uint64_t> first(n_packs);
    std::vector<uint32_t> count(n_packs), prefix(n_packs);
    uint32_t at = 0;
    for (uint64_t p = 0; p < n_packs; ++p) {
        first[p] = ranges[p].first, count[p] = ranges[p].count, prefix[p] = at;
        at += ranges[p].count;  // <= n < 2^32 - 1: the ranges do not overlap
    }
    if (rcdc_status rs = pr->first.ensure(std::max<uint64_t>(n_packs, 1), true)) return rs;
    if (rcdc_status rs = pr->count.ensure(std::max<uint64_t>(n_packs, 1), true)) return rs;
    if (rcdc_status rs = pr->prefix.ensure(std::max<uint64_t>(n_packs, 1), true)) return rs;
    if (rcdc_status rs = pr->hits.ensure(std::max<uint64_t>(n, 1), true)) return rs;
    if (rcdc_status rs = pr->pack_of.ensure(std::max<uint64_t>(n, 1), true)) return rs;
    if (n_packs) {
        HIP_TRY(hipMemcpyAsync(pr->first, first.data(), n_packs * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(pr->count, count.data(), n_packs * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(pr->prefix, prefix.data(), n_packs * 4, hipMemcpyHostToDevice, st));
    }
    if (n) {
        const uint8_t *ids = (const uint8_t *)d_ids;
        if (id_stride != 32 || ((uintptr_t)d_ids & 15u)) {
            if (rcdc_status rs = pr->ids.ensure(n * 32, true)) return rs;
            hipLaunchKernelGGL(rcdc_pr_gather_ids_kernel, dim3(blocks_for(n * 8)), dim3(kBlock), 0,
                               st, ids, id_stride, n, pr->ids);
            HIP_TRY(hipGetLastError());
            ids = pr->ids;
        }
        HIP_TRY(hipMemsetAsync(pr->pack_of, 0xFF, n * 4, st));
        if (n_packs) {
            hipLaunchKernelGGL(rcdc_pr_pack_of_kernel, dim3((uint32_t)n_packs), dim3(kBlock), 0, st,
                               pr->first, pr->count, n,
                               pr->pack_of);
            HIP_TRY(hipGetLastError());
        }
        if (rcdc_status rs = rcdc_dindex_lookup(pr->dx, ids, n, pr->hits, st))
            return rs;
    }
    // the host vectors above must outlive their copies
    HIP_TRY(hipStreamSynchronize(st));
    pr->have_entries = true;
    return RCDC_OK;
}

rcdc_status rcdc_prune_mark(rcdc_prune *pr, uint8_t *d_counts, uint8_t *d_used,
                            rcdc_prune_pack *packs, rcdc_prune_result *result,
                            void *hip_stream) {
    if (!pr) return invalid("rcdc_prune_mark: handle is NULL");
    if (!result) return invalid("rcdc_prune_mark: result is NULL");
    std::lock_guard<std::mutex> lk(pr->mu);
    if (!pr->have_entries) return invalid("rcdc_prune_mark: no entries set");
    const uint64_t n = pr->n, m = pr->m, np = pr->n_packs;
    if ((m && !d_counts) || (n && !d_used) || (np && !packs))
        return invalid("rcdc_prune_mark: null array");
    DeviceGuard g(pr->device);
    hipStream_t st = (hipStream_t)hip_stream;
    const PrView v = view_of(pr);

    // scalars: [0] missing, [1] dup entries, [2] compaction cursor, [3] unsettled,
    // [4] (as uint32) first missing
    if (rcdc_status rs = pr->scalars.ensure(5, true)) return rs;
    unsigned long long *sc = pr->scalars;
    uint32_t *first_missing = reinterpret_cast<uint32_t *>(sc + 4);
    if (rcdc_status rs = pr->cnt.ensure(std::max<uint64_t>(m, 1), true)) return rs;
    if (rcdc_status rs = pr->taken.ensure(std::max<uint64_t>(m, 1), true)) return rs;
    if (rcdc_status rs = pr->state.ensure(std::max<uint64_t>(np, 1), true)) return rs;
    if (rcdc_status rs = pr->pending.ensure(std::max<uint64_t>(np, 1), true)) return rs;
    if (rcdc_status rs = pr->trigger.ensure(std::max<uint64_t>(np, 1), true)) return rs;
    if (rcdc_status rs = pr->packs_out.ensure(std::max<uint64_t>(np, 1), true)) return rs;
    uint32_t *cnt = pr->cnt, *taken = pr->taken;
    uint32_t *state = pr->state, *pending = pr->pending;
    uint32_t *trigger = pr->trigger;

    HIP_TRY(hipEventRecord(pr->ev[0], st));
    HIP_TRY(hipMemsetAsync(sc, 0, 4 * 8, st));
    HIP_TRY(hipMemsetAsync(sc + 4, 0xFF, 8, st));
    if (m) {
        HIP_TRY(hipMemsetAsync(cnt, 0, m * 4, st));
        HIP_TRY(hipMemsetAsync(taken, 0xFF, m * 4, st));
    }
    if (np) {
        HIP_TRY(hipMemsetAsync(state, 0, np * 4, st));
        HIP_TRY(hipMemsetAsync(pending, 0, np * 4, st));
        HIP_TRY(hipMemsetAsync(trigger, 0xFF, np * 4, st));
    }
    if (n) {
        hipLaunchKernelGGL(rcdc_pr_count_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, st, v, cnt);
        HIP_TRY(hipGetLastError());
    }
    if (m) {
        hipLaunchKernelGGL(rcdc_pr_counts_out_kernel, dim3(blocks_for(m)), dim3(kBlock), 0, st, cnt,
                           m, d_counts, sc, first_missing);
        HIP_TRY(hipGetLastError());
    }
    if (n) {
        hipLaunchKernelGGL(rcdc_pr_singles_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, st, v, cnt,
                           d_used, state, trigger, sc + 1);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long host_sc[5];
    HIP_TRY(hipMemcpyAsync(host_sc, sc, sizeof host_sc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t nd = host_sc[1];
    uint32_t rounds = 0;
    if (nd) {
        if (rcdc_status rs = pr->keys_a.ensure(nd, true)) return rs;
        if (rcdc_status rs = pr->keys_b.ensure(nd, true)) return rs;
        if (rcdc_status rs = pr->vals_a.ensure(nd, true)) return rs;
        if (rcdc_status rs = pr->vals_b.ensure(nd, true)) return rs;
        if (rcdc_status rs = pr->progress.ensure(nd, true)) return rs;
        uint64_t *ka = pr->keys_a, *kb = pr->keys_b;
        uint32_t *va = pr->vals_a, *vb = pr->vals_b;
        hipLaunchKernelGGL(rcdc_pr_compact_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, st, v, cnt,
                           sc + 2, nd, ka, va);
        HIP_TRY(hipGetLastError());
        size_t tmp = 0;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp, ka, kb, va, vb, (size_t)nd, 0u, 64u, st));
        if (rcdc_status rs = pr->sort_tmp.ensure(std::max<uint64_t>(tmp, 1), true)) return rs;
        HIP_TRY(rocprim::radix_sort_pairs(pr->sort_tmp, tmp, ka, kb, va, vb, (size_t)nd, 0u, 64u,
                                         st));
        HIP_TRY(hipMemsetAsync(pr->progress, 0, nd * 4, st));
        hipLaunchKernelGGL(rcdc_pr_pending_kernel, dim3(blocks_for(nd)), dim3(kBlock), 0, st, v, kb,
                           vb, nd, cnt, pending);
        HIP_TRY(hipGetLastError());
    }
    if (np) {
        hipLaunchKernelGGL(rcdc_pr_idle_packs_kernel, dim3(blocks_for(np)), dim3(kBlock), 0, st, np,
                           pending, state);
        HIP_TRY(hipGetLastError());
    }
    if (nd) {
        const uint64_t *kb = pr->keys_b;
        const uint32_t *vb = pr->vals_b;
        for (;;) {
            if (rounds > np)  // n_packs + 1 rounds have run and ids are still unsettled
                return rcdc::set_error(RCDC_ERR_INTERNAL,
                                       "rcdc_prune_mark: the marking did not settle");
            HIP_TRY(hipMemsetAsync(sc + 3, 0, 8, st));
            hipLaunchKernelGGL(rcdc_pr_round_kernel, dim3(blocks_for(nd)), dim3(kBlock), 0, st, v,
                               kb, vb, nd, cnt, taken, pr->progress, state, pending,
                               trigger, sc + 3);
            HIP_TRY(hipGetLastError());
            ++rounds;
            unsigned long long unsettled = 0;
            HIP_TRY(hipMemcpyAsync(&unsettled, sc + 3, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (!unsettled) break;
        }
        hipLaunchKernelGGL(rcdc_pr_flags_kernel, dim3(blocks_for(nd)), dim3(kBlock), 0, st, v, kb,
                           vb, nd, taken, trigger, d_used);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(pr->ev[1], st));
    if (np) {
        hipLaunchKernelGGL(rcdc_pr_sums_kernel, dim3((uint32_t)((np + 3) / 4)), dim3(kBlock), 0, st,
                           v, d_used, pr->len, pr->len_stride, pr->ulen, pr->ulen_stride,
                           pr->packs_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(packs, pr->packs_out, np * sizeof(rcdc_prune_pack),
                              hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipEventRecord(pr->ev[2], st));
    HIP_TRY(hipStreamSynchronize(st));
    result->missing = host_sc[0];
    result->first_missing = (uint32_t)host_sc[4];
    result->dup_entries = nd;
    result->rounds = rounds;
    result->pad = 0;
    HIP_TRY(hipEventElapsedTime(&result->mark_ms, pr->ev[0], pr->ev[1]));
    HIP_TRY(hipEventElapsedTime(&result->sums_ms, pr->ev[1], pr->ev[2]));
    return RCDC_OK;
}

rcdc_status rcdc_prune_keep(rcdc_prune *pr, const uint8_t *kinds, const uint32_t *file_rank,
                            uint8_t *d_keep, void *hip_stream) {
    if (!pr) return invalid("rcdc_prune_keep: handle is NULL");
    std::lock_guard<std::mutex> lk(pr->mu);
    if (!pr->have_entries) return invalid("rcdc_prune_keep: no entries set");
    const uint64_t n = pr->n, m = pr->m, np = pr->n_packs;
    if ((np && (!kinds || !file_rank)) || (n && !d_keep)) return invalid("rcdc_prune_keep: null array");
    // file order: pack by rank, then the file position of each pack's first entry
    std::vector<uint32_t> by_rank(np, kNone), fprefix(np);
    for (uint64_t p = 0; p < np; ++p) {
        if (kinds[p] > RCDC_PRUNE_REPACK) return invalid("rcdc_prune_keep: unknown pack kind");
        if (file_rank[p] >= np || by_rank[file_rank[p]] != kNone)
            return invalid("rcdc_prune_keep: file_rank is no permutation");
        by_rank[file_rank[p]] = (uint32_t)p;
    }
    uint32_t at = 0;
    for (uint64_t r = 0; r < np; ++r) {
        fprefix[by_rank[r]] = at;
        at += pr->ranges[by_rank[r]].count;
    }
    if (n == 0) return RCDC_OK;
    DeviceGuard g(pr->device);
    hipStream_t st = (hipStream_t)hip_stream;
    const PrView v = view_of(pr);
    if (rcdc_status rs = pr->kinds.ensure(std::max<uint64_t>(np, 1), true)) return rs;
    if (rcdc_status rs = pr->fprefix.ensure(std::max<uint64_t>(np, 1), true)) return rs;
    if (rcdc_status rs = pr->blocked.ensure(std::max<uint64_t>(m, 1), true)) return rs;
    if (rcdc_status rs = pr->minpos.ensure(std::max<uint64_t>(m, 1), true)) return rs;
    if (np) {
        HIP_TRY(hipMemcpyAsync(pr->kinds, kinds, np, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(pr->fprefix, fprefix.data(), np * 4, hipMemcpyHostToDevice, st));
        // the host vector must outlive its copy (pageable memory is staged
        // before the call returns, but do not rely on it)
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (m) {
        HIP_TRY(hipMemsetAsync(pr->blocked, 0, m * 4, st));
        HIP_TRY(hipMemsetAsync(pr->minpos, 0xFF, m * 4, st));
    }
    hipLaunchKernelGGL(rcdc_pr_keep_a_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, st, v,
                       pr->kinds, pr->fprefix,
                       pr->blocked, pr->minpos);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rcdc_pr_keep_b_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, st, v,
                       pr->kinds, pr->fprefix,
                       pr->blocked, pr->minpos, d_keep);
    HIP_TRY(hipGetLastError());
    return RCDC_OK;
}

}  // extern "C"
