// rcdc_place_blobs (include/rcdc.h): decoded blobs scattered to their file
// positions -- the byte work of restore_contents after
// read_encrypted_from_partial (commands/restore.rs:630-668): one blob
// written to each of its 1..k destinations, and SparseRestore::ByContent's
// `data.iter().all(|&b| b == 0)` over the same bytes.
//
// A blob is cut into tiles of at most 64 KiB of source (rcdc_place.h), one
// workgroup each, so an 8 MiB chunk is 128 workgroups' work.  Lane t of a
// round owns the 16-aligned source granule j = j0 + t: it loads the granule
// once, takes granule j + 1 from the next lane (lane 63 loads it), feeds the
// zero test with its own granule, and for every destination stores the one
// 16-aligned destination chunk whose first byte lies in granule j -- the
// funnel of rcdc_copy_ranges_kernel (v_alignbit over five dwords), with a
// shift that is uniform per destination.  The destination's ragged head and
// tail (< 16 bytes each) go byte by byte.  Loads touch granules 0 .. G-1 of
// the tile only (the granules that contain source bytes); stores stay inside
// [dest, dest + len).
//
// This unit is its own translation unit on purpose: nothing here is shared
// with rcdc_zstd_dec.hip / rcdc_zstd_dx.hip.

#include "rcdc_place.h"

namespace {

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

// bytes [lo, hi) of a granule kept, the others cleared (0 <= lo <= hi <= 16)
__device__ __forceinline__ u32x4v keep_bytes(u32x4v v, uint32_t lo, uint32_t hi) {
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t l = lo > 4 * k ? min(lo - 4 * k, 4u) : 0u;
        const uint32_t h = hi > 4 * k ? min(hi - 4 * k, 4u) : 0u;
        uint32_t m = 0;
        if (h > l) {
            m = h == 4 ? 0xFFFFFFFFu : (1u << (8 * h)) - 1u;
            m &= l == 0 ? 0xFFFFFFFFu : ~((1u << (8 * l)) - 1u);
        }
        w[k] &= m;
    }
    u32x4v r;
    r.x = w[0]; r.y = w[1]; r.z = w[2]; r.w = w[3];
    return r;
}

// 16 bytes from byte 4 * kk + rr / 8 of the 32 bytes A || B
__device__ __forceinline__ u32x4v funnel(u32x4v A, u32x4v B, uint32_t kk, uint32_t rr) {
    uint32_t x0, x1, x2, x3, x4;
    if (kk == 0) {
        x0 = A.x; x1 = A.y; x2 = A.z; x3 = A.w; x4 = B.x;
    } else if (kk == 1) {
        x0 = A.y; x1 = A.z; x2 = A.w; x3 = B.x; x4 = B.y;
    } else if (kk == 2) {
        x0 = A.z; x1 = A.w; x2 = B.x; x3 = B.y; x4 = B.z;
    } else {
        x0 = A.w; x1 = B.x; x2 = B.y; x3 = B.z; x4 = B.w;
    }
    u32x4v v;
    v.x = __builtin_amdgcn_alignbit(x1, x0, rr);
    v.y = __builtin_amdgcn_alignbit(x2, x1, rr);
    v.z = __builtin_amdgcn_alignbit(x3, x2, rr);
    v.w = __builtin_amdgcn_alignbit(x4, x3, rr);
    return v;
}

__device__ __forceinline__ u32x4v nbr(u32x4v A) {
    u32x4v B;
    B.x = __shfl_down(A.x, 1);
    B.y = __shfl_down(A.y, 1);
    B.z = __shfl_down(A.z, 1);
    B.w = __shfl_down(A.w, 1);
    return B;
}

}  // namespace

template <bool WRITE, bool ZERO>
__global__ __launch_bounds__(256) void rcdc_place_kernel(const rcdc::PlaceTile *__restrict__ tiles,
                                                         uint32_t n,
                                                         const uint64_t *__restrict__ daddr,
                                                         uint32_t *nz, uint32_t skip) {
    const uint32_t t = threadIdx.x, ln = t & 63u;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const rcdc::PlaceTile T = tiles[k];
        uint32_t nd = WRITE ? T.ndests : 0u;
        if (WRITE && skip && nz[T.blob] == 0u) nd = 0u;  // an all-zero blob is not written
        if (!ZERO && nd == 0u) continue;
        const uint64_t off = T.off & ~rcdc::kPlaceAligned;
        const bool shuf = nd != 0u && !(T.off & rcdc::kPlaceAligned);
        const uint8_t *s = reinterpret_cast<const uint8_t *>((uintptr_t)T.src);
        const uint32_t len = T.len;
        const uint32_t a = (uint32_t)T.src & 15u;
        const u32x4v *s16 = reinterpret_cast<const u32x4v *>(s - a);
        const uint32_t G = (a + len + 15u) >> 4;  // granules that hold source bytes
        const uint32_t e = (a + len) & 15u;       // bytes of the last granule in range (0: all)
        // ragged ends of every destination: fewer than 16 bytes each
        for (uint32_t d = 0; d < nd; d++) {
            uint8_t *dp = reinterpret_cast<uint8_t *>((uintptr_t)(daddr[T.dest0 + d] + off));
            uint32_t head = (16u - ((uint32_t)(uintptr_t)dp & 15u)) & 15u;
            if (head > len) head = len;
            if (t < head) dp[t] = s[t];
            const uint32_t done = head + ((len - head) & ~15u);
            if (t < len - done) dp[done + t] = s[done + t];
        }
        uint32_t acc = 0;
        for (uint32_t j0 = 0; j0 < G; j0 += 1024u) {
            u32x4v A[4], B[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t j = j0 + 256u * q + t;
                A[q] = u32x4v{0u, 0u, 0u, 0u};
                B[q] = A[q];
                if (j < G) A[q] = __builtin_nontemporal_load(s16 + j);
                if (shuf && ln == 63u && j + 1u < G) B[q] = __builtin_nontemporal_load(s16 + j + 1u);
            }
            if (shuf) {
                // every lane of the wave runs the shuffle; a lane past the
                // last granule holds zeros
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const u32x4v N = nbr(A[q]);
                    if (ln != 63u) B[q] = N;
                }
            }
            if (ZERO) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t j = j0 + 256u * q + t;
                    u32x4v m = A[q];
                    // bytes of the first and last granule outside the blob
                    // take no part
                    if (j < G && ((j == 0u && a) || (j + 1u == G && e)))
                        m = keep_bytes(m, j == 0u ? a : 0u, (j + 1u == G && e) ? e : 16u);
                    acc |= m.x | m.y | m.z | m.w;
                }
            }
            for (uint32_t d = 0; d < nd; d++) {
                const uint64_t dp = daddr[T.dest0 + d] + off;
                uint32_t head = (16u - ((uint32_t)dp & 15u)) & 15u;
                if (head > len) head = len;
                const uint32_t body = (len - head) >> 4;
                // destination chunk i starts at source byte head + 16 i, which
                // is byte sh of granule i + o
                const uint32_t ah = a + head, o = ah >> 4, sh = ah & 15u;
                const uint32_t kk = sh >> 2, rr = (sh & 3u) * 8u;
                u32x4v *db = reinterpret_cast<u32x4v *>((uintptr_t)(dp + head));
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t j = j0 + 256u * q + t;
                    if (j >= o && j - o < body)
                        __builtin_nontemporal_store(funnel(A[q], B[q], kk, rr), db + (j - o));
                }
            }
        }
        if (ZERO) {
            // idempotent: any wave that saw a non-zero byte stores the same 1
            if (__ballot(acc != 0u) != 0ull && ln == 0u) nz[T.blob] = 1u;
        }
    }
}

namespace rcdc {

hipError_t launch_place(const PlaceTile *tiles, uint32_t n, const uint64_t *daddr, uint32_t *nz,
                        bool write, bool zero, bool skip, uint32_t cus, hipStream_t stream) {
    if (n == 0 || (!write && !zero)) return hipSuccess;
    const uint32_t g = n < cus * 8u ? n : cus * 8u;
    const uint32_t sk = skip ? 1u : 0u;
    if (write && zero)
        hipLaunchKernelGGL((rcdc_place_kernel<true, true>), dim3(g), dim3(256), 0, stream, tiles, n,
                           daddr, nz, sk);
    else if (write)
        hipLaunchKernelGGL((rcdc_place_kernel<true, false>), dim3(g), dim3(256), 0, stream, tiles,
                           n, daddr, nz, sk);
    else
        hipLaunchKernelGGL((rcdc_place_kernel<false, true>), dim3(g), dim3(256), 0, stream, tiles,
                           n, daddr, nz, sk);
    return hipGetLastError();
}

}  // namespace rcdc
