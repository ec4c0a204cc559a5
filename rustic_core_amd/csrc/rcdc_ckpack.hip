// rcdc_check_packs (include/rcdc.h): the kernels.  A pack is the work of one
// workgroup of four waves in each of three passes:
//   judge   a workgroup per pack: reads the pack's entries once, in input
//           order: are they in order, and if so the findings' counts, the end
//           offset and the header length.  A pack out of order leaves as soon
//           as a tile shows it.
//   sort    only for the packs judge found out of order and small enough:
//           (offset, length, uncompressed length, input position) in LDS, a
//           bitonic network over the next power of two, then the same counts
//           in sorted order.  The input position as the last key makes the
//           order total, so equal locations keep input order.
//   number  an exclusive scan of the findings per pack (one workgroup).
//   emit    only for packs with findings, a header to compare, or when the
//           caller wants the order: the records at their scanned places.
// sort and emit have work for few packs, so each walks a list of its packs
// (written in pack order by a scan: sort_list, number) with a grid of fixed
// size instead of a workgroup per pack that ends at once.
// Every value a lane reads from another was written before a barrier or a
// kernel boundary; the LDS atomics are integer sums and minima, so the result
// does not depend on their order.

#include "rcdc_ckpack.h"

namespace rcdc {
namespace {

struct CkKey {
    uint32_t off, len, ulen;
};

__device__ inline CkKey ck_key(const CkEntries &e, uint64_t i) {
    if (e.loc_records) {
        const uint4 v = *reinterpret_cast<const uint4 *>(e.off - 4 + i * 16);
        return {v.y, v.z, v.w};
    }
    return {*reinterpret_cast<const uint32_t *>(e.off + i * e.off_stride),
            *reinterpret_cast<const uint32_t *>(e.len + i * e.len_stride),
            *reinterpret_cast<const uint32_t *>(e.ulen + i * e.ulen_stride)};
}

__device__ inline uint32_t ck_type(const CkEntries &e, uint64_t i, uint32_t ptype) {
    return e.types ? e.types[i] : ptype;
}

__device__ inline bool ck_less(const CkKey &a, const CkKey &b) {
    if (a.off != b.off) return a.off < b.off;
    if (a.len != b.len) return a.len < b.len;
    return a.ulen < b.ulen;
}

__device__ inline bool ck_less4(const uint4 &a, const uint4 &b) {
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    if (a.z != b.z) return a.z < b.z;
    return a.w < b.w;
}

// inclusive scan of v over the workgroup (wrapping); total: the sum of all.
// Every thread of the workgroup calls it; s_w holds one word per wave.
__device__ inline uint32_t ck_scan(uint32_t v, uint32_t *s_w, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    __syncthreads();  // the last call's readers are through
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    uint32_t add = 0, tot = 0;
    for (uint32_t i = 0; i < kCkBlock / 64; i++) {
        const uint32_t x = s_w[i];
        if (i < w) add += x;
        tot += x;
    }
    total = tot;
    return v + add;
}

// the pack's type: its first entry's in input order; without type bytes the
// header's, or data
__device__ inline uint32_t ck_pack_type(const CkArgs &a, uint32_t p, const rcdc_prune_range &r) {
    if (a.e.types) return r.count ? a.e.types[r.first] : 0u;
    if (a.hdrs && a.hdrs[p].type != RCDC_CKPACK_NO_HEADER) return a.hdrs[p].type;
    return 0u;
}

__device__ inline void ck_write_pack(const CkArgs &a, uint32_t p, uint32_t status, uint32_t type,
                                     uint32_t sorted, const uint32_t *acc, uint32_t end,
                                     uint32_t count) {
    rcdc_ckpack_pack o = {};
    o.status = status;
    o.type = type;
    if (status == RCDC_CKPACK_OK) {
        o.type_findings = acc[0];
        o.offset_findings = acc[1];
        o.end_offset = end;
        o.sorted = sorted;
        o.header_len = 32ull + 37ull * count + 4ull * acc[2];
    }
    a.packs[p] = o;
}

__global__ __launch_bounds__(kCkBlock) void rcdc_ck_judge_kernel(CkArgs a) {
    __shared__ uint32_t s_w[kCkBlock / 64];
    __shared__ uint32_t s_acc[4];
    const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const rcdc_prune_range r = a.ranges[p];
    const uint32_t ptype = ck_pack_type(a, p, r);
    if (tid < 4) s_acc[tid] = 0;
    uint32_t carry = 0, nt = 0, no = 0, n41 = 0;
    int unsorted = 0;
    for (uint64_t base = 0; base < r.count; base += kCkBlock) {
        const uint64_t k = base + tid;
        const bool live = k < r.count;
        CkKey key = {0, 0, 0};
        if (live) key = ck_key(a.e, r.first + k);
        // the entry before: the lane below, or a load for a wave's first lane
        CkKey prev = {__shfl_up(key.off, 1, 64), __shfl_up(key.len, 1, 64),
                      __shfl_up(key.ulen, 1, 64)};
        if (live && lane == 0 && k) prev = ck_key(a.e, r.first + k - 1);
        uint32_t tot;
        const uint32_t incl = ck_scan(live ? key.len : 0u, s_w, tot);
        if (live) {
            if (k && ck_less(key, prev)) unsorted = 1;
            nt += ck_type(a.e, r.first + k, ptype) != ptype;
            no += key.off != carry + incl - key.len;
            n41 += key.ulen != 0;
        }
        carry += tot;
        unsorted = __syncthreads_or(unsorted);
        if (unsorted) break;
    }
    if (unsorted) {
        if (tid == 0)
            ck_write_pack(a, p, r.count <= kCkSortMax ? kCkNeedsSort : RCDC_CKPACK_HOST, ptype, 0,
                          s_acc, 0, 0);
        return;
    }
    __syncthreads();  // s_acc is zero
    if (nt) atomicAdd(&s_acc[0], nt);
    if (no) atomicAdd(&s_acc[1], no);
    if (n41) atomicAdd(&s_acc[2], n41);
    __syncthreads();
    if (tid == 0) ck_write_pack(a, p, RCDC_CKPACK_OK, ptype, 1, s_acc, carry, r.count);
}

// one pack of the sort list, by the whole workgroup
__device__ inline void ck_sort_pack(const CkArgs &a, uint32_t p, uint4 *s_k, uint32_t *s_w,
                                    uint32_t *s_acc) {
    const uint32_t tid = threadIdx.x;
    const rcdc_prune_range r = a.ranges[p];
    const uint32_t n = r.count;  // 2 .. kCkSortMax
    const uint32_t ptype = a.packs[p].type;
    uint32_t m = 2;
    while (m < n) m <<= 1;
    if (tid < 4) s_acc[tid] = 0;
    for (uint32_t i = tid; i < m; i += kCkBlock) {
        uint4 v = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, i};  // padding: behind every entry
        if (i < n) {
            const CkKey key = ck_key(a.e, r.first + i);
            v.x = key.off, v.y = key.len, v.z = key.ulen;
        }
        s_k[i] = v;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < m / 2; t += kCkBlock) {
                const uint32_t lo = 2 * t - (t & (j - 1)), hi = lo + j;
                const bool up = (lo & k) == 0;
                const uint4 x = s_k[lo], y = s_k[hi];
                if (ck_less4(y, x) == up) {
                    s_k[lo] = y;
                    s_k[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    const uint32_t at = a.prefix[p];
    uint32_t carry = 0, nt = 0, no = 0, n41 = 0;
    for (uint32_t base = 0; base < n; base += kCkBlock) {
        const uint32_t k = base + tid;
        const bool live = k < n;
        const uint4 v = live ? s_k[k] : uint4{0, 0, 0, 0};
        uint32_t tot;
        const uint32_t incl = ck_scan(live ? v.y : 0u, s_w, tot);
        if (live) {
            a.order_tmp[at + k] = v.w;
            nt += ck_type(a.e, r.first + v.w, ptype) != ptype;
            no += v.x != carry + incl - v.y;
            n41 += v.z != 0;
        }
        carry += tot;
    }
    __syncthreads();
    if (nt) atomicAdd(&s_acc[0], nt);
    if (no) atomicAdd(&s_acc[1], no);
    if (n41) atomicAdd(&s_acc[2], n41);
    __syncthreads();
    if (tid == 0) ck_write_pack(a, p, RCDC_CKPACK_OK, ptype, 0, s_acc, carry, n);
}

// the packs of the sort list, a workgroup at a time: the grid does not grow
// with the packs, most of which are in order
__global__ __launch_bounds__(kCkBlock) void rcdc_ck_sort_kernel(CkArgs a) {
    __shared__ uint4 s_k[kCkSortMax];
    __shared__ uint32_t s_w[kCkBlock / 64];
    __shared__ uint32_t s_acc[4];
    const uint32_t count = a.list_n[0];
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        ck_sort_pack(a, a.list[i], s_k, s_w, s_acc);
        __syncthreads();  // the record is written: LDS is free again
    }
}

constexpr uint32_t kCkNumber = 1024;

// inclusive scan of v over a workgroup of kCkNumber threads; total: the sum
__device__ inline uint64_t ck_scan_wide(uint64_t v, uint64_t *s_w, uint64_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= d) v += t;
    }
    __syncthreads();
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    uint64_t add = 0, tot = 0;
    for (uint32_t i = 0; i < kCkNumber / 64; i++) {
        const uint64_t x = s_w[i];
        if (i < w) add += x;
        tot += x;
    }
    total = tot;
    return v + add;
}

// the packs judge found out of order and small enough, in pack order
__global__ __launch_bounds__(kCkNumber) void rcdc_ck_sort_list_kernel(CkArgs a) {
    __shared__ uint64_t s_w[kCkNumber / 64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < a.n_packs; base += kCkNumber) {
        const uint64_t p = base + threadIdx.x;
        const bool mine = p < a.n_packs && a.packs[p].status == kCkNeedsSort;
        uint64_t tot;
        const uint64_t incl = ck_scan_wide(mine, s_w, tot);
        if (mine) a.list[carry + incl - 1] = (uint32_t)p;
        carry += tot;
    }
    if (threadIdx.x == 0) a.list_n[0] = (uint32_t)carry;
}

__global__ __launch_bounds__(kCkNumber) void rcdc_ck_number_kernel(CkArgs a) {
    __shared__ uint64_t s_w[kCkNumber / 64];
    __shared__ uint32_t s_cnt[2];
    const uint32_t tid = threadIdx.x;
    if (tid < 2) s_cnt[tid] = 0;
    uint64_t carry = 0, listed = 0;
    uint32_t host = 0, here = 0;
    for (uint64_t base = 0; base < a.n_packs; base += kCkNumber) {
        const uint64_t p = base + tid;
        uint64_t mine = 0;
        bool ok = false, emit = false;
        if (p < a.n_packs) {
            const rcdc_ckpack_pack &o = a.packs[p];
            ok = o.status == RCDC_CKPACK_OK;
            if (ok) {
                mine = (uint64_t)o.type_findings + o.offset_findings;
                here += o.sorted == 0;
                // what the emit pass has work for: findings, the order, a header
                emit = mine != 0 || a.order != nullptr ||
                       (a.hdrs && a.hdrs[p].type != RCDC_CKPACK_NO_HEADER);
            } else {
                host++;
            }
        }
        uint64_t tot;
        const uint64_t incl = ck_scan_wide(mine, s_w, tot);
        if (ok) a.packs[p].first_finding = carry + incl - mine;
        carry += tot;
        const uint64_t at = ck_scan_wide(emit, s_w, tot);
        if (emit) a.list[listed + at - 1] = (uint32_t)p;
        listed += tot;
    }
    __syncthreads();
    if (host) atomicAdd(&s_cnt[0], host);
    if (here) atomicAdd(&s_cnt[1], here);
    __syncthreads();
    if (tid == 0) {
        a.totals[0] = carry;
        a.totals[1] = s_cnt[0];
        a.totals[2] = s_cnt[1];
        a.list_n[1] = (uint32_t)listed;
    }
}

// the 32 id bytes of an entry against a header row's (16-byte aligned)
__device__ inline bool ck_id_equal(const CkEntries &e, uint64_t i, const uint8_t *row) {
    const uint8_t *id = e.ids + i * e.id_stride;
    if (e.id_rows) {
        const uint4 a0 = reinterpret_cast<const uint4 *>(id)[0];
        const uint4 a1 = reinterpret_cast<const uint4 *>(id)[1];
        const uint4 b0 = reinterpret_cast<const uint4 *>(row)[0];
        const uint4 b1 = reinterpret_cast<const uint4 *>(row)[1];
        return a0.x == b0.x && a0.y == b0.y && a0.z == b0.z && a0.w == b0.w && a1.x == b1.x &&
               a1.y == b1.y && a1.z == b1.z && a1.w == b1.w;
    }
    bool same = true;
    for (uint32_t b = 0; b < 32; b++) same &= id[b] == row[b];
    return same;
}

// one pack of the emit list, by the whole workgroup
__device__ inline void ck_emit_pack(const CkArgs &a, uint32_t p, uint32_t *s_w, uint32_t &s_min) {
    const uint32_t tid = threadIdx.x;
    const rcdc_ckpack_pack rec = a.packs[p];
    if (rec.status != RCDC_CKPACK_OK) return;  // the whole workgroup
    rcdc_ckpack_hdr h = {RCDC_CKPACK_NO_HEADER, 0, 0};
    if (a.hdrs) h = a.hdrs[p];
    const bool has_h = h.type != RCDC_CKPACK_NO_HEADER;
    const bool has_f = rec.type_findings != 0 || rec.offset_findings != 0;
    if (!has_f && !has_h && !a.order) return;
    const rcdc_prune_range r = a.ranges[p];
    const uint32_t at = a.prefix[p], ptype = rec.type;
    if (tid == 0) s_min = 0xFFFFFFFFu;
    __syncthreads();
    uint32_t carry = 0;
    uint64_t fbase = rec.first_finding;
    for (uint64_t base = 0; base < r.count; base += kCkBlock) {
        const uint64_t k = base + tid;
        const bool live = k < r.count;
        uint64_t e = 0;
        if (live) {
            e = r.first + (rec.sorted ? k : (uint64_t)a.order_tmp[at + k]);
            if (a.order) a.order[r.first + k] = (uint32_t)e;
        }
        if (!has_f && !has_h) continue;
        CkKey key = {0, 0, 0};
        uint32_t type = ptype;
        if (live) {
            key = ck_key(a.e, e);
            type = ck_type(a.e, e, ptype);
        }
        if (has_f) {
            uint32_t tot;
            const uint32_t incl = ck_scan(live ? key.len : 0u, s_w, tot);
            const uint32_t expected = carry + incl - key.len;
            carry += tot;
            const uint32_t ft = live && type != ptype, fo = live && key.off != expected;
            const uint32_t c_incl = ck_scan(ft + fo, s_w, tot);
            uint64_t pos = fbase + c_incl - (ft + fo);
            fbase += tot;
            if (ft) {
                if (pos < a.cap_findings)
                    a.findings[pos] = {p, (uint32_t)e, RCDC_CKPACK_TYPE, type, ptype};
                pos++;
            }
            if (fo && pos < a.cap_findings)
                a.findings[pos] = {p, (uint32_t)e, RCDC_CKPACK_OFFSET, key.off, expected};
        }
        if (has_h && live && k < h.count) {
            const uint64_t j = h.first + k;
            const uint4 hl = *reinterpret_cast<const uint4 *>(a.hdr_locs[h.type] + j);
            const bool same = hl.y == key.off && hl.z == key.len && hl.w == key.ulen &&
                              type == h.type && ck_id_equal(a.e, e, a.hdr_ids[h.type] + j * 32);
            if (!same) atomicMin(&s_min, (uint32_t)k);
        }
    }
    if (!has_h) return;
    __syncthreads();
    if (tid == 0) {
        uint32_t diff = s_min;
        if (h.count != r.count) diff = min(diff, min(h.count, r.count));
        a.packs[p].header_verdict = diff == 0xFFFFFFFFu ? RCDC_CKPACK_EQUAL : RCDC_CKPACK_DIFFERS;
        a.packs[p].header_diff = diff == 0xFFFFFFFFu ? 0u : diff;
    }
}

__global__ __launch_bounds__(kCkBlock) void rcdc_ck_emit_kernel(CkArgs a) {
    __shared__ uint32_t s_w[kCkBlock / 64];
    __shared__ uint32_t s_min;
    const uint32_t count = a.list_n[1];
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        ck_emit_pack(a, a.list[i], s_w, s_min);
        __syncthreads();  // s_min was read
    }
}

}  // namespace

hipError_t launch_ck_packs(const CkArgs &a, hipStream_t st) {
    if (!a.n_packs) return hipSuccess;
    hipLaunchKernelGGL(rcdc_ck_judge_kernel, dim3(a.n_packs), dim3(kCkBlock), 0, st, a);
    // sort and emit walk their lists with a grid that does not grow with the packs
    hipLaunchKernelGGL(rcdc_ck_sort_list_kernel, dim3(1), dim3(kCkNumber), 0, st, a);
    hipLaunchKernelGGL(rcdc_ck_sort_kernel, dim3(a.n_packs < 1024u ? a.n_packs : 1024u),
                       dim3(kCkBlock), 0, st, a);
    hipLaunchKernelGGL(rcdc_ck_number_kernel, dim3(1), dim3(kCkNumber), 0, st, a);
    hipLaunchKernelGGL(rcdc_ck_emit_kernel, dim3(a.n_packs < 4096u ? a.n_packs : 4096u),
                       dim3(kCkBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace rcdc
