// rcdc_index_write (include/rcdc.h): entry arrays in HBM -> the JSON text of
// index files, the bytes serde_json::to_vec(&IndexFile) writes.  gfx950,
// wave64.  The parser's stages (rcdc_ixparse.hip) in reverse.
//
// Stage 1, sizes.  One lane per WRITTEN entry w (the blobs of all written
// packs in output order; wfirst[p] of them come before pack p): the lane
// finds its pack, reads the entry's three integers and stores the length of
// its object, its leading comma included.  A device scan turns the lengths
// into epos[w], the bytes of entries before w.
//
// Stage 2, packs and files.  One lane per pack: its framing plus
// epos[wfirst[p + 1]] - epos[wfirst[p]]; a second scan gives ppos[p].  One
// wave then walks the files: a file's length is its root text plus the
// ppos difference of its packs, its offset the running sum of the lengths
// rounded up to 16.  One lane per pack stores where the pack begins in
// d_out (pabs) and the constant that turns epos[w] into the place of entry w
// (ebase).
//
// Stage 3, emit.  One wave owns a span of kIxwSpan bytes of d_out.  It finds
// by binary search the files, the packs and the entries that touch the span
// (places grow with the file, pack and entry number); its lanes format those
// objects into LDS at their places within the span, an object that crosses
// the span's edge clipped to it (its other part is the neighbouring wave's);
// then the span leaves with one 16-byte store per lane and row.  Files begin
// on 16-byte boundaries, so a 16-byte chunk is wholly a file's, or a file's
// ragged end (stored byte by byte), or no file's (not stored).  Hex digits
// and decimal digits are made in registers.

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "rcdc_ixwrite.h"
#include "rcdc_wave.h"

namespace {

using namespace rcdc;

struct Widen {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

__device__ __forceinline__ uint32_t ndigits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) +
           (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}

__device__ __forceinline__ uint32_t load_u32(const uint8_t *base, uint64_t stride, uint64_t e) {
    return *reinterpret_cast<const uint32_t *>(base + e * stride);
}

// The pack of written entry w among packs [lo, hi): the last p with
// wfirst[p] <= w (so a pack without blobs is never the answer).  The caller
// knows wfirst[lo] <= w < wfirst[hi].
__device__ __forceinline__ uint32_t pack_of(const uint32_t *wfirst, uint32_t lo, uint32_t hi,
                                            uint32_t w) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (wfirst[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t pack_tail_len(const IxwPack &pk) {
    return 2u + ((pk.flags & kIxwTime) ? 10u + pk.time_len : 0u) +
           ((pk.flags & kIxwSize) ? 8u + ndigits(pk.size) : 0u);
}

// ---- stage 1 -------------------------------------------------------------------

__global__ __launch_bounds__(kIxwBlock) void ixw_sizes(IxwArgs a) {
    const uint64_t w64 = (uint64_t)blockIdx.x * kIxwBlock + threadIdx.x;
    if (w64 > a.n_written) return;
    const uint32_t w = (uint32_t)w64;
    if (w == a.n_written) {
        a.sizes[w] = 0;
        return;
    }
    const uint32_t p = pack_of(a.wfirst, 0, a.n_packs, w);
    const uint32_t k = w - a.wfirst[p];
    const uint64_t e = a.packs[p].first + k;
    const uint32_t ulen = load_u32(a.ulen, a.ulen_stride, e);
    a.sizes[w] = kIxwBlobFixed + ndigits(load_u32(a.off, a.off_stride, e)) +
                 ndigits(load_u32(a.len, a.len_stride, e)) + (ulen ? ndigits(ulen) : 4u) +
                 (k ? 1u : 0u);
}

// ---- stage 2 -------------------------------------------------------------------

__global__ __launch_bounds__(kIxwBlock) void ixw_packs(IxwArgs a) {
    const uint64_t p64 = (uint64_t)blockIdx.x * kIxwBlock + threadIdx.x;
    if (p64 > a.n_packs) return;
    const uint32_t p = (uint32_t)p64;
    if (p == a.n_packs) {
        a.psize[p] = 0;
        return;
    }
    const IxwPack pk = a.packs[p];
    a.psize[p] = ((pk.flags & kIxwComma) ? 1u : 0u) + kIxwPackHead +
                 (a.epos[a.wfirst[p + 1]] - a.epos[a.wfirst[p]]) + pack_tail_len(pk);
}

// one wave: the files' lengths and their 16-byte aligned offsets
__global__ __launch_bounds__(64) void ixw_files(IxwArgs a) {
    const uint32_t lane = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < a.n_files; base += 64) {
        const uint32_t f = base + lane;
        uint64_t len = 0;
        if (f < a.n_files) {
            const IxwFile fl = a.files[f];
            len = (uint64_t)fl.head_len + (a.ppos[fl.pack_b] - a.ppos[fl.pack_a]) + fl.mid_len + 2u;
        }
        const uint64_t pad = (len + 15u) & ~15ull;
        const uint64_t incl = wave_incl_add64(pad);
        const uint64_t off = carry + incl - pad;
        if (f < a.n_files) {
            a.fout[f].off = off;
            a.fout[f].len = len;
            if (f == a.n_files - 1) *a.total = off + len;
        }
        carry += shfl64(incl, 63);
    }
}

__global__ __launch_bounds__(kIxwBlock) void ixw_place(IxwArgs a) {
    const uint64_t p64 = (uint64_t)blockIdx.x * kIxwBlock + threadIdx.x;
    if (p64 >= a.n_packs) return;
    const uint32_t p = (uint32_t)p64;
    const IxwPack pk = a.packs[p];
    const IxwFile fl = a.files[pk.file];
    const uint64_t at = a.fout[pk.file].off + fl.head_len + (a.ppos[p] - a.ppos[fl.pack_a]) +
                        ((pk.flags & kIxwDelete) ? fl.mid_len : 0u);
    a.pabs[p] = at;
    a.ebase[p] = at + ((pk.flags & kIxwComma) ? 1u : 0u) + kIxwPackHead - a.epos[a.wfirst[p]];
}

// ---- stage 3 -------------------------------------------------------------------

// Writes text into a span's LDS image.  rel is the next byte's place counted
// from the span's first byte; with CLIP a byte outside the span is dropped.
template <bool CLIP>
struct Put {
    uint8_t *lds;
    int32_t rel;

    __device__ __forceinline__ void c(uint8_t b) {
        if (!CLIP || (uint32_t)rel < kIxwSpan) lds[rel] = b;
        rel++;
    }
    template <uint32_t N>
    __device__ __forceinline__ void s(const char (&t)[N]) {
#pragma unroll
        for (uint32_t i = 0; i + 1 < N; i++) c((uint8_t)t[i]);
    }
    __device__ __forceinline__ void dec(uint32_t v) {
        const uint32_t n = ndigits(v);
        for (uint32_t i = n; i-- > 0;) {
            const uint32_t q = v / 10u;
            const int32_t at = rel + (int32_t)i;
            if (!CLIP || (uint32_t)at < kIxwSpan) lds[at] = (uint8_t)('0' + (v - q * 10u));
            v = q;
        }
        rel += (int32_t)n;
    }
    __device__ __forceinline__ void hex(uint8_t b) {
        const uint32_t h = b >> 4, l = b & 15u;
        c((uint8_t)(h + (h < 10u ? '0' : 'a' - 10)));
        c((uint8_t)(l + (l < 10u ? '0' : 'a' - 10)));
    }
    // an id held as 8 little-endian words
    __device__ __forceinline__ void id(const uint32_t (&w)[8]) {
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) hex((uint8_t)(w[i] >> (8 * j)));
    }
};

template <bool CLIP>
__device__ __forceinline__ void put_blob(Put<CLIP> o, const uint32_t (&id)[8], bool tree,
                                         bool comma, uint32_t off, uint32_t len, uint32_t ulen) {
    if (comma) o.c(',');
    o.s("{\"id\":\"");
    o.id(id);
    o.s("\",\"type\":\"");
    if (tree) o.s("tree"); else o.s("data");
    o.s("\",\"offset\":");
    o.dec(off);
    o.s(",\"length\":");
    o.dec(len);
    o.s(",\"uncompressed_length\":");
    if (ulen) o.dec(ulen); else o.s("null");
    o.c('}');
}

// whether [at, at + n) meets the span [s0, s0 + kIxwSpan)
__device__ __forceinline__ bool meets(uint64_t at, uint64_t n, uint64_t s0) {
    return n && at + n > s0 && at < s0 + kIxwSpan;
}

// the last i < n with offs(i) <= x; the caller knows offs(0) <= x
template <class F>
__device__ __forceinline__ uint32_t last_le(F offs, uint32_t lo, uint32_t hi, uint64_t x) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offs(mid) <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void ixw_emit(IxwArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kIxwSpan];
    const uint64_t total = *a.total;
    const uint64_t s0 = (uint64_t)blockIdx.x * kIxwSpan;
    if (s0 >= total) return;
    const uint64_t s1 = s0 + kIxwSpan;
    const uint32_t lane = threadIdx.x;
    auto file_off = [&](uint32_t f) { return a.fout[f].off; };
    auto pack_at = [&](uint32_t p) { return a.pabs[p]; };

    // ---- the blobs and the packs' own text -----------------------------------
    uint32_t p_lo = 0, p_hi = 0;  // the packs that may touch the span
    if (a.n_packs && a.pabs[0] < s1) {
        p_lo = a.pabs[0] > s0 ? 0u : last_le(pack_at, 0, a.n_packs, s0);
        p_hi = last_le(pack_at, 0, a.n_packs, s1 - 1) + 1u;
    }
    if (p_hi > p_lo) {
        // the first entry of pack p_lo that ends behind s0, and the first of
        // pack p_hi - 1 that begins at s1 or later
        uint32_t w_lo = a.wfirst[p_lo], hi = a.wfirst[p_lo + 1];
        const uint64_t eb_lo = a.ebase[p_lo];
        while (w_lo < hi) {
            const uint32_t mid = w_lo + (hi - w_lo) / 2;
            if (eb_lo + a.epos[mid + 1] > s0) hi = mid; else w_lo = mid + 1;
        }
        uint32_t w_hi = a.wfirst[p_hi - 1];
        hi = a.wfirst[p_hi];
        const uint64_t eb_hi = a.ebase[p_hi - 1];
        while (w_hi < hi) {
            const uint32_t mid = w_hi + (hi - w_hi) / 2;
            if (eb_hi + a.epos[mid] >= s1) hi = mid; else w_hi = mid + 1;
        }
        const bool words = (((uintptr_t)a.ids | a.id_stride) & 3u) == 0;
        for (uint64_t w64 = (uint64_t)w_lo + lane; w64 < w_hi; w64 += 64) {
            const uint32_t w = (uint32_t)w64;
            const uint32_t p = pack_of(a.wfirst, p_lo, p_hi, w);
            const uint32_t k = w - a.wfirst[p];
            const uint64_t e = a.packs[p].first + k;
            const bool tree = (a.packs[p].flags & kIxwTree) != 0;
            const int32_t rel = (int32_t)(int64_t)(a.ebase[p] + a.epos[w] - s0);
            const uint32_t size = a.sizes[w];
            uint32_t id[8];
            const uint8_t *src = a.ids + e * a.id_stride;
            if (words) {
#pragma unroll
                for (int i = 0; i < 8; i++) id[i] = reinterpret_cast<const uint32_t *>(src)[i];
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++)
                    id[i] = (uint32_t)src[4 * i] | ((uint32_t)src[4 * i + 1] << 8) |
                            ((uint32_t)src[4 * i + 2] << 16) | ((uint32_t)src[4 * i + 3] << 24);
            }
            const uint32_t off = load_u32(a.off, a.off_stride, e);
            const uint32_t len = load_u32(a.len, a.len_stride, e);
            const uint32_t ulen = load_u32(a.ulen, a.ulen_stride, e);
            if (rel >= 0 && (uint32_t)rel + size <= kIxwSpan)
                put_blob(Put<false>{lds, rel}, id, tree, k != 0, off, len, ulen);
            else
                put_blob(Put<true>{lds, rel}, id, tree, k != 0, off, len, ulen);
        }
        for (uint64_t p64 = (uint64_t)p_lo + lane; p64 < p_hi; p64 += 64) {
            const uint32_t p = (uint32_t)p64;
            const IxwPack pk = a.packs[p];
            const uint64_t at = a.pabs[p];
            const uint32_t head = ((pk.flags & kIxwComma) ? 1u : 0u) + kIxwPackHead;
            if (meets(at, head, s0)) {
                Put<true> o{lds, (int32_t)(int64_t)(at - s0)};
                if (pk.flags & kIxwComma) o.c(',');
                o.s("{\"id\":\"");
                o.id(pk.id);
                o.s("\",\"blobs\":[");
            }
            const uint32_t tail = pack_tail_len(pk);
            const uint64_t tat = at + (a.ppos[p + 1] - a.ppos[p]) - tail;
            if (meets(tat, tail, s0)) {
                Put<true> o{lds, (int32_t)(int64_t)(tat - s0)};
                o.c(']');
                if (pk.flags & kIxwTime) {
                    o.s(",\"time\":\"");
                    for (uint32_t i = 0; i < pk.time_len; i++) o.c(a.times[pk.time_off + i]);
                    o.c('"');
                }
                if (pk.flags & kIxwSize) {
                    o.s(",\"size\":");
                    o.dec(pk.size);
                }
                o.c('}');
            }
        }
    }

    // ---- the roots' own text ---------------------------------------------------
    const uint32_t f_lo = last_le(file_off, 0, a.n_files, s0);
    const uint32_t f_hi = last_le(file_off, f_lo, a.n_files, s1 - 1);
    for (uint64_t f64 = (uint64_t)f_lo + lane; f64 <= f_hi; f64 += 64) {
        const uint32_t f = (uint32_t)f64;
        const IxwFile fl = a.files[f];
        const uint64_t at = a.fout[f].off;
        if (meets(at, fl.head_len, s0)) {
            Put<true> o{lds, (int32_t)(int64_t)(at - s0)};
            o.c('{');
            if (fl.has_sup) {
                o.s("\"supersedes\":[");
                // id k and the comma behind it are the kIxwSupId bytes at
                // ids + kIxwSupId * k: only those that meet the span
                const uint64_t ids = at + 15u;
                const uint64_t k0 = s0 > ids ? (s0 - ids) / kIxwSupId : 0u;
                const uint64_t k1 = s1 > ids ? (s1 - ids + kIxwSupId - 1) / kIxwSupId : 0u;
                for (uint64_t k = k0; k < k1 && k < fl.sup_count; k++) {
                    o.rel = (int32_t)(int64_t)(ids + k * kIxwSupId - s0);
                    o.c('"');
                    const uint8_t *src = a.sup + ((uint64_t)fl.sup_first + k) * 32u;
                    for (int i = 0; i < 32; i++) o.hex(src[i]);
                    o.c('"');
                    if (k + 1 < fl.sup_count) o.c(',');
                }
                o.rel = (int32_t)(int64_t)(at + fl.head_len - 11u - s0);
                o.s("],");
            }
            o.s("\"packs\":[");
        }
        const uint64_t mat = at + fl.head_len + (a.ppos[fl.pack_b - fl.n_delete] - a.ppos[fl.pack_a]);
        if (meets(mat, fl.mid_len, s0)) {
            Put<true> o{lds, (int32_t)(int64_t)(mat - s0)};
            o.s("],\"packs_to_delete\":[");
        }
        const uint64_t tat = at + a.fout[f].len - 2u;
        if (meets(tat, 2, s0)) {
            Put<true> o{lds, (int32_t)(int64_t)(tat - s0)};
            o.s("]}");
        }
    }
    __syncthreads();

    // ---- the span leaves -----------------------------------------------------------
    for (uint32_t c = lane; c < kIxwChunks; c += 64) {
        const uint64_t at = s0 + 16u * c;
        if (at >= total) break;
        const uint32_t f = last_le(file_off, f_lo, f_hi + 1, at);
        const uint64_t end = a.fout[f].off + a.fout[f].len;
        if (at >= end) continue;  // the gap in front of the next file
        if (end - at >= 16u) {
            *reinterpret_cast<u32x4v *>(a.out + at) = *reinterpret_cast<const u32x4v *>(lds + 16u * c);
        } else {
            const uint32_t n = (uint32_t)(end - at);
            for (uint32_t j = 0; j < n; j++) a.out[at + j] = lds[16u * c + j];
        }
    }
}

}  // namespace

namespace rcdc {

hipError_t ix_write_scan_bytes(uint64_t n, size_t *bytes) {
    size_t b1 = 0, b2 = 0;
    hipError_t e = rocprim::exclusive_scan(
        nullptr, b1, rocprim::make_transform_iterator((const uint32_t *)nullptr, Widen()),
        (uint64_t *)nullptr, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>());
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(nullptr, b2, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>());
    *bytes = b1 > b2 ? b1 : b2;
    return e;
}

hipError_t launch_ix_write(const IxwArgs &a, hipStream_t st) {
    const uint64_t nw = (uint64_t)a.n_written + 1, np = (uint64_t)a.n_packs + 1;
    size_t tmp = a.scan_tmp_bytes;
    ixw_sizes<<<dim3((uint32_t)((nw + kIxwBlock - 1) / kIxwBlock)), dim3(kIxwBlock), 0, st>>>(a);
    hipError_t e = rocprim::exclusive_scan(a.scan_tmp, tmp,
                                           rocprim::make_transform_iterator(
                                               (const uint32_t *)a.sizes, Widen()),
                                           a.epos, (uint64_t)0, (size_t)nw,
                                           rocprim::plus<uint64_t>(), st);
    if (e != hipSuccess) return e;
    ixw_packs<<<dim3((uint32_t)((np + kIxwBlock - 1) / kIxwBlock)), dim3(kIxwBlock), 0, st>>>(a);
    tmp = a.scan_tmp_bytes;
    e = rocprim::exclusive_scan(a.scan_tmp, tmp, (const uint64_t *)a.psize, a.ppos, (uint64_t)0,
                                (size_t)np, rocprim::plus<uint64_t>(), st);
    if (e != hipSuccess) return e;
    ixw_files<<<dim3(1), dim3(64), 0, st>>>(a);
    if (a.n_packs)
        ixw_place<<<dim3((a.n_packs + kIxwBlock - 1) / kIxwBlock), dim3(kIxwBlock), 0, st>>>(a);
    if (a.n_spans) ixw_emit<<<dim3(a.n_spans), dim3(64), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace rcdc
