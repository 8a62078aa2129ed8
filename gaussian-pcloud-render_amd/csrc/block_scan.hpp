// block_scan.hpp -- the wave and workgroup prefix sums shared by sort.hip and density_control.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// inclusive wave64 scan via shuffles (not hot)
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t n = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += n;
    }
    return v;
}

// exclusive scan of one value per thread across a 256-thread workgroup; tmp = 4 words of LDS
__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t* tmp, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    if (lane == 63) tmp[w] = inc;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if ((uint32_t)i < w) base += tmp[i];
    if (total) *total = tmp[0] + tmp[1] + tmp[2] + tmp[3];
    __syncthreads();
    return base + inc - v;
}

}  // namespace gsr
