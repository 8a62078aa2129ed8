// render_walk.hpp -- what the render kernels (render_fwd.hip: k_render_forward<NX>, k_render_forward_half; render_bwd.hip:
// k_render_backward<MODE, NX, ...>) share.  All three: the hand-retired prefetch loads, the instrumentation macros (stats.hpp) and the host
// helpers (the vector types and exp_nonpos come with render_math.hpp).  k_render_forward_half and k_render_backward also the quadrant
// geometry and the wave maximum; k_render_forward<NX> keeps its own copies of those two, because its machine code moves with the shared ones
// (profiles/r10_render_walk_refactor.txt, which also records why the gather pipeline itself is still written out per kernel).
#pragma once

#include "common.hpp"
#include "render_math.hpp"
#include "stats.hpp"

namespace gsr {

// Prefetch loads are issued as inline asm so that hipcc's waitcnt pass does not see them: left to itself it puts
// an s_waitcnt for the NEXT round's records inside the CURRENT round's evaluation loop and re-exposes the gather
// latency every 64 entries.  The loads are retired by hand with one s_waitcnt vmcnt(0) at the rotation point; that
// asm takes the destination registers as in/out operands, so nothing can read them earlier.
__device__ __forceinline__ void prefetch16(f32x4& dst, const void* p)
{
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void prefetch4(uint32_t& dst, const void* p)
{
    asm volatile("global_load_dword %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void prefetch4f(float& dst, const void* p)
{
    asm volatile("global_load_dword %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void retire_prefetch(f32x4& a, f32x4& b, float& c, uint32_t& d)
{
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}
__device__ __forceinline__ void retire_prefetch_x(f32x4& a, f32x4& b, float& c, uint32_t& d, f32x4& e, f32x4& f)
{
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f)::"memory");
}

// Where a wave's pixels are: quadrant q of `tile` (8 x 8 pixels from (x0, y0); the half-quadrant forward passes the pixel index
// of its 8 x 4 half and the half's row offset), this lane's pixel and whether it lies in the image.  (Results come back through
// references here and in wave_max_of: returned by value, the same arithmetic reaches the register allocator in another order
// and the kernels' machine code moves.)
struct QuadGeom {
    uint32_t x0, y0, px, py;
    bool inside;
    float pixf_x, pixf_y, x0f, y0f;
};
__device__ __forceinline__ void quad_geom(QuadGeom& g, uint32_t tile, uint32_t q, int gridx, int W, int H, uint32_t pl, uint32_t row_off = 0u)
{
    const uint32_t tx = tile % (uint32_t)gridx, ty = tile / (uint32_t)gridx;
    g.x0 = tx * TILE_X + (q & 1u) * 8u;
    g.y0 = ty * TILE_Y + (q >> 1) * 8u + row_off;
    g.px = g.x0 + (pl & 7u);
    g.py = g.y0 + (pl >> 3);
    g.inside = g.px < (uint32_t)W && g.py < (uint32_t)H;
    g.pixf_x = (float)g.px; g.pixf_y = (float)g.py;
    g.x0f = (float)g.x0; g.y0f = (float)g.y0;
}

// v becomes the largest v of the wave's 64 lanes, in every lane
__device__ __forceinline__ void wave_max_of(uint32_t& v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = v > o ? v : o;
    }
}

// host side: what the forward's and the backward's argument structs take alike from a submission -- image, tile grid, slice
// length, views and the strides between their arenas
template <typename ARGS>
inline void set_frame_args(ARGS& a, const gsr_params& p, const Batch& B)
{
    a.W = p.W; a.H = p.H;
    a.gridx = (p.W + TILE_X - 1) / TILE_X;
    a.num_tiles = a.gridx * ((p.H + TILE_Y - 1) / TILE_Y);
    a.chunk_shift = B.chunk_shift();
    a.V = (uint32_t)B.V;
    a.g_stride = B.g_stride; a.b_stride = B.b_stride; a.iv_stride = B.iv_stride;
}

}  // namespace gsr
