// rcdc_wave.h -- the wave and workgroup helpers of the parsers and judges
// (rcdc_ixparse.hip, rcdc_trparse.hip, rcdc_pkhdr.hip, rcdc_ixwrite.hip,
// rcdc_cktree.hip), one copy.  Device only, wave64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rcdc {

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_incl_add64(uint64_t v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)v, d, 64);
        const uint32_t hi = __shfl_up((uint32_t)(v >> 32), d, 64);
        if (lane >= d) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// lane src's v
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
    const uint32_t lo = __shfl((uint32_t)v, src, 64);
    const uint32_t hi = __shfl((uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// One workgroup of 1024, a record of four uint32 per thread: the sum of the
// records of the threads before this one, and *all: of all 1024.
__device__ inline u32x4v block_excl4(u32x4v x, u32x4v *lds /* 16 */, u32x4v *all) {
    const uint32_t lane = lane_id(), wave = threadIdx.x / 64;
    u32x4v inc;
    inc.x = wave_incl_add(x.x);
    inc.y = wave_incl_add(x.y);
    inc.z = wave_incl_add(x.z);
    inc.w = wave_incl_add(x.w);
    __syncthreads();  // a call before this one has read lds
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    u32x4v before = {0u, 0u, 0u, 0u}, sum = {0u, 0u, 0u, 0u};
    for (uint32_t w = 0; w < 16; w++) {
        const u32x4v s = lds[w];
        if (w < wave) before += s;
        sum += s;
    }
    *all = sum;
    return before + inc - x;
}

// Exclusive scan of n records of four uint32 in place, the totals to v[n]:
// one workgroup of 1024, a chunk of 1024 records per pass.
__device__ inline void block_scan4(u32x4v *v, uint32_t n, u32x4v *lds /* 16 */) {
    u32x4v carry = {0u, 0u, 0u, 0u};
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        u32x4v x = {0u, 0u, 0u, 0u};
        if (i < n) x = v[i];
        u32x4v all;
        const u32x4v before = block_excl4(x, lds, &all);
        if (i < n) v[i] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) v[n] = carry;
}

// workgroups of `per` items for n items
static inline uint32_t blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// launches on the stream `st` of the calling function, which returns the
// launch's error if there is one
#define RCDC_LAUNCH(kernel, grid, block, ...)                                      \
    do {                                                                           \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);   \
        if (hipError_t e_ = hipGetLastError(); e_ != hipSuccess) return e_;        \
    } while (0)

}  // namespace rcdc
