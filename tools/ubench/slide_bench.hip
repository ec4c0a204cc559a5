// Byte-step cost of the shipped Rabin64 inner loop and its variants, timed
// alternately in one process.  Every case is rcdc_slide.h's own code (the
// header is included, not restated): scan_segment over a 4-unit register ring
// with the outgoing bytes 64 back, tables in 32 LDS copies, one workgroup per
// CU.  The data is a few hundred KB that every wave re-reads (L2 hits), so the
// figure is the loop's, not HBM's.
//
//   V0     slide<K, 105>, G = 116, 16 waves              (the parent's loop)
//   V0r0   V0 with the rare path never entered (no lane counts)
//   T1     G = 216: v_and_b32 + v_min3_u32, exact at any mask width
//   A      slide<K, 205>: MOD address in one v_lshrrev_b32_sdwa
//   A16    A with G = 16 (the group's fingerprints kept, no re-roll)
//   V16    V0 with G = 16
//   A16m   A16 with one v_min_u16 per byte as the prefilter (G = 1016)
//   V16m   V16 with it
//   W12    V0 at 12 waves per CU
//   W12x2  12 waves, two chains per lane over half segments (64 more warm-up
//          bytes per lane)
//   A12x2  W12x2 on the A slide
//
// usage: slide_bench [rounds]        alternating rounds, min and median
//        slide_bench pmc             one launch per case (for rocprofv3 --pmc)
// ns per wave-byte per CU counts the tested bytes (S per lane), so a case pays
// for its own warm-up.  tools/ubench/slide_counts.py adds the instruction
// counts from the disassembly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rustic_core_amd/csrc/rcdc_slide.h"

namespace {

constexpr uint32_t kS = 1536;        // the walk's segment
constexpr uint32_t kRegions = 8;     // distinct data regions the waves read
constexpr uint32_t kShifts = 16;     // per-rep start offsets (64 bytes apart)
constexpr uint32_t kRegionBytes = 64u * kS + 64u + kShifts * 64u;

// ---- two chains per lane ---------------------------------------------------
template <int TSH, int GG>
__device__ __forceinline__ void scan_unit2(Chain &a, Chain &b, const Unit &an, const Unit &ao,
                                           const Unit &bn, const Unit &bo, const uint8_t *tab,
                                           const Consts &k, bool lv, uint32_t rb) {
#pragma unroll
    for (int g = 0; g < 64 / GG; g++) {
        const uint32_t a0 = a.h0, a1 = a.h1, b0 = b.h0, b1 = b.h1;
        uint16_t acca = 0xFFFFu, accb = 0xFFFFu;
#pragma unroll
        for (int j = 0; j < GG; j++) {
            const int p = g * GG + j;
            slide_b<TSH>(p, a.h0, a.h1, UDW(an, p >> 2), UDW(ao, p >> 2), tab, k);
            slide_b<TSH>(p, b.h0, b.h1, UDW(bn, p >> 2), UDW(bo, p >> 2), tab, k);
            acca = __builtin_elementwise_min(acca, (uint16_t)a.h0);
            accb = __builtin_elementwise_min(accb, (uint16_t)b.h0);
        }
        if (acca == 0 && lv) rescan_group<TSH, GG>(a, a0, a1, an, ao, tab, k, rb + g * GG, g);
        if (accb == 0 && lv) rescan_group<TSH, GG>(b, b0, b1, bn, bo, tab, k, rb + g * GG, g);
    }
}

template <int TSH, int GG, int B>
__device__ __forceinline__ bool ring2_step(Chain &a, Chain &b, Unit (&ua)[4], Unit (&ub)[4],
                                           uint32_t &i, uint32_t nunits,
                                           __amdgpu_buffer_rsrc_t rsrc, uint32_t va, uint32_t vb,
                                           const uint8_t *tab, const Consts &k, bool lv) {
    scan_unit2<TSH, GG>(a, b, ua[B], ua[(B + 3) % 4], ub[B], ub[(B + 3) % 4], tab, k, lv,
                        (i - 1) * 64u);
    if ((B & 1) == 0) {
        const uint32_t nxt = i + 2;
        if (nxt <= nunits) {
            load_unit(ua[(B + 2) % 4], rsrc, va + nxt * 64u);
            load_unit(ua[(B + 3) % 4], rsrc, va + (nxt + 1) * 64u);
            load_unit(ub[(B + 2) % 4], rsrc, vb + nxt * 64u);
            load_unit(ub[(B + 3) % 4], rsrc, vb + (nxt + 1) * 64u);
        }
    }
    return ++i <= nunits;
}

// Both chains test `nunits` units: a from va, b from vb (each after its own
// 64 warm-up bytes).  Loads past a chain's last unit stay inside the buffer.
template <int TSH, int GG>
__device__ __forceinline__ void scan_segment2(Chain &a, Chain &b, __amdgpu_buffer_rsrc_t rsrc,
                                              uint32_t va, uint32_t vb, uint32_t nunits,
                                              const uint8_t *tab, const Consts &k, bool lv) {
    Unit ua[4], ub[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        load_unit(ua[j], rsrc, va + j * 64u);
        load_unit(ub[j], rsrc, vb + j * 64u);
    }
    warm_unit<TSH>(a, ua[0], tab, k);
    warm_unit<TSH>(b, ub[0], tab, k);
    uint32_t i = 1;
    for (;;) {
        if (!ring2_step<TSH, GG, 1>(a, b, ua, ub, i, nunits, rsrc, va, vb, tab, k, lv)) break;
        if (!ring2_step<TSH, GG, 2>(a, b, ua, ub, i, nunits, rsrc, va, vb, tab, k, lv)) break;
        if (!ring2_step<TSH, GG, 3>(a, b, ua, ub, i, nunits, rsrc, va, vb, tab, k, lv)) break;
        if (!ring2_step<TSH, GG, 0>(a, b, ua, ub, i, nunits, rsrc, va, vb, tab, k, lv)) break;
    }
}

__device__ __forceinline__ Chain new_chain(uint32_t rhi) {
    Chain c;
    c.h0 = c.h1 = 0;
    c.first = c.last = kNone;
    c.count = 0;
    c.rlo = 0;
    c.rhi = rhi;
    return c;
}

}  // namespace

// NC chains per lane; RARE false: no lane counts, so the rare path is never
// entered (its rate forced to 0 on the same data).
template <int TSH, int G, int WAVES, int NC, bool RARE>
__global__ __launch_bounds__(WAVES * 64, 1) void slide_kern(const uint8_t *__restrict__ data,
                                                            uint32_t data_bytes,
                                                            const uint64_t *__restrict__ gtab,
                                                            uint32_t reps, uint32_t mask,
                                                            uint32_t *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tab[kLdsBytes];
    fill_tables(s_tab, gtab, 21u, threadIdx.x, WAVES * 64);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Consts k = make_consts(lane, mask, 21u);
    const uint32_t region = (blockIdx.x * WAVES + wave) % kRegions;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(data + region * kRegionBytes), (short)0,
        (int)(data_bytes - region * kRegionBytes), 0x00020000);
    const uint64_t valid = RARE ? ~0ull : (uint64_t)(mask == 0u);  // 0, unknown to the compiler
    uint32_t acc = 0;
    for (uint32_t r = 0; r < reps; r++) {
        const uint32_t voff = lane * kS + (r % kShifts) * 64u;
        if constexpr (NC == 1) {
            const Chain c = scan_segment<4, true, TSH, false, G>(rsrc, voff, kS / 64u, 0u, kS, s_tab,
                                                                 k, valid, lane);
            acc += c.first ^ c.last ^ c.count ^ c.h0 ^ c.h1;
        } else {
            Chain a = new_chain(kS / 2), b = new_chain(kS / 2);
            scan_segment2<TSH, G - 100>(a, b, rsrc, voff, voff + kS / 2, kS / 128u, s_tab, k,
                                        valid != 0);
            // the lane's summary, as one chain would report it
            const uint32_t first = a.first != kNone ? a.first
                                   : b.first != kNone ? b.first + kS / 2 : kNone;
            const uint32_t last = b.last != kNone ? b.last + kS / 2 : a.last;
            acc += first ^ last ^ (a.count + b.count) ^ b.h0 ^ b.h1;
        }
    }
    out[blockIdx.x * WAVES * 64 + threadIdx.x] = acc;
}

namespace {

// Rabin tables of the default polynomial (degree 53), the layout the kernels
// take: OUT[256] then MOD[256].
constexpr uint64_t kPoly = 0x3DA3358B4DC173ull;
uint64_t pmod(uint64_t x) {
    for (int b = 63; b >= 53; b--)
        if (x >> b & 1) x ^= kPoly << (b - 53);
    return x;
}
void build_tables(uint64_t *t) {
    for (uint64_t b = 0; b < 256; b++) {
        uint64_t h = pmod(b);
        for (int i = 0; i < 63; i++) h = pmod(h << 8);
        t[b] = h;
        t[256 + b] = pmod(b << 53) | (b << 53);
    }
}

struct Case {
    const char *name;
    const void *fn;
    int waves, nc;
    void (*launch)(int, const uint8_t *, uint32_t, const uint64_t *, uint32_t, uint32_t, uint32_t *);
    std::vector<float> ms;
};

template <int TSH, int G, int WAVES, int NC, bool RARE>
void launch(int cus, const uint8_t *d, uint32_t n, const uint64_t *gt, uint32_t reps, uint32_t mask,
            uint32_t *out) {
    hipLaunchKernelGGL((slide_kern<TSH, G, WAVES, NC, RARE>), dim3(cus), dim3(WAVES * 64), 0, 0, d, n,
                       gt, reps, mask, out);
}
template <int TSH, int G, int WAVES, int NC, bool RARE>
Case make(const char *name) {
    return Case{name, (const void *)slide_kern<TSH, G, WAVES, NC, RARE>, WAVES, NC,
                launch<TSH, G, WAVES, NC, RARE>, {}};
}

#define CK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));            \
            return 1;                                                          \
        }                                                                      \
    } while (0)

}  // namespace

int main(int argc, char **argv) {
    const bool pmc = argc > 1 && !strcmp(argv[1], "pmc");
    const int rounds = pmc ? 1 : (argc > 1 ? std::max(atoi(argv[1]), 5) : 7);
    const uint32_t reps = 8, mask = 0xFFFFFu;
    hipDeviceProp_t pr;
    CK(hipGetDeviceProperties(&pr, 0));
    const int cus = pr.multiProcessorCount;
    uint64_t ht[512];
    build_tables(ht);
    uint64_t *gt;
    CK(hipMalloc(&gt, sizeof ht));
    CK(hipMemcpy(gt, ht, sizeof ht, hipMemcpyHostToDevice));
    const uint32_t nbytes = kRegions * kRegionBytes + 4096u;
    std::vector<uint8_t> hd(nbytes);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto &b : hd) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        b = (uint8_t)(x >> 32);
    }
    uint8_t *dd;
    CK(hipMalloc(&dd, nbytes));
    CK(hipMemcpy(dd, hd.data(), nbytes, hipMemcpyHostToDevice));
    uint32_t *out;
    CK(hipMalloc(&out, (size_t)cus * 1024 * 4));

    std::vector<Case> cs;
    cs.push_back(make<105, 116, 16, 1, true>("V0"));
    cs.push_back(make<105, 116, 16, 1, false>("V0r0"));
    cs.push_back(make<105, 216, 16, 1, true>("T1"));
    cs.push_back(make<205, 116, 16, 1, true>("A"));
    cs.push_back(make<205, 16, 16, 1, true>("A16"));
    cs.push_back(make<105, 16, 16, 1, true>("V16"));
    cs.push_back(make<205, 1016, 16, 1, true>("A16m"));
    cs.push_back(make<105, 1016, 16, 1, true>("V16m"));
    cs.push_back(make<105, 116, 12, 1, true>("W12"));
    cs.push_back(make<105, 116, 12, 2, true>("W12x2"));
    cs.push_back(make<205, 116, 12, 2, true>("A12x2"));

    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<uint32_t> ho((size_t)cus * 1024);
    for (auto &c : cs) {  // warm-up launch, and the output's checksum
        CK(hipMemset(out, 0, ho.size() * 4));
        c.launch(cus, dd, nbytes, gt, reps, mask, out);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(ho.data(), out, ho.size() * 4, hipMemcpyDeviceToHost));
        uint32_t sum = 0;
        for (size_t i = 0; i < (size_t)cus * c.waves * 64; i++) sum += ho[i] * (uint32_t)(i % 64 + 1);
        hipFuncAttributes fa;
        CK(hipFuncGetAttributes(&fa, c.fn));
        printf("# %-6s waves %2d chains %d vgprs %3d scratch %zu B lane0..63 checksum %08x\n", c.name,
               c.waves, c.nc, fa.numRegs, (size_t)fa.localSizeBytes, sum);
    }
    if (pmc) return 0;
    for (int r = 0; r < rounds; r++)
        for (auto &c : cs) {
            CK(hipEventRecord(e0));
            c.launch(cus, dd, nbytes, gt, reps, mask, out);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            c.ms.push_back(ms);
        }
    printf("%d CUs, %d rounds, %u reps of %u tested bytes per lane\n", cus, rounds, reps, kS);
    printf("%-6s %5s %6s  %9s %9s  (ns per wave-byte per CU)  vs V0 min\n", "case", "waves",
           "chains", "min", "median");
    double v0 = 0;
    for (auto &c : cs) {
        std::sort(c.ms.begin(), c.ms.end());
        const double per = 1e6 / ((double)c.waves * reps * kS);
        const double mn = c.ms.front() * per, md = c.ms[c.ms.size() / 2] * per;
        if (v0 == 0) v0 = mn;
        printf("%-6s %5d %6d  %9.3f %9.3f  %+.1f %%\n", c.name, c.waves, c.nc, mn, md,
               100.0 * (mn / v0 - 1.0));
    }
    return 0;
}
