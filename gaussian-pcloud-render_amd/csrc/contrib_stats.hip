// contrib_stats.hip -- what every Gaussian contributes to the rendered pixels: a read-only walk of the lists a forward left in the
// arenas.  Importance-based pruning ranks a Gaussian by its blend weights w = alpha T; only the compositing loop
// knows them.  Per Gaussian i, over the V views of the submission, with an optional per-pixel weight map m (m = 1 without one; a value
// with !(m > 0) -- negative, zero, NaN -- is 0 and masks its pixel out of all four statistics):
//   weight_sum[i]     = sum over (view, pixel) contributions of w m          weight_max[i] = the largest w m
//   pixel_count[i]    = number of (view, pixel) contributions               dominant_count[i] = number of (view, pixel) where i has the
//                                                                            largest w of the pixel (strict >: the front-most wins a tie)
// A contribution is what the exact-mode forward blends: not power > 0, not alpha < 1/255, and T (1 - alpha) >= 1e-4 (the entry that
// takes a pixel below 1e-4 stops it and is not blended), pixels inside the image only.  The arithmetic is ALWAYS the exact mode's
// (render_math.hpp power_exact / alpha_exact, T (1 - alpha) one rounding at a time), whatever gsr_set_render_math and
// gsr_set_train_math say: the decisions are those of an exact forward bit for bit.  Nothing the forward stored per pixel is read --
// inference forwards store neither final_T nor n_contrib -- the walk carries T and the done flag itself.
//
// Mapping: the forward's.  One wave64 = one 8x8 quadrant of a tile, single-wave workgroups, tiles in the forward's work order, groups
// of 32 workgroups dealt to the views round-robin.  A round is 64 list entries, one per lane: gather the Splat record (the next round's
// records and the ids of the round after are in flight meanwhile), drop what the exact-safe footprint test (tile_cull.hpp) proves
// cannot reach 1/255 in the box of the pixels still live, stage the survivors compacted in the wave's own LDS (two 16-B words per
// entry, read back with same-address ds_read_b128: no barrier, DS operations of one wave execute in order).
//
// Reduction: an entry's 64 per-pixel values are reduced inside the wave before anything leaves it -- a ballot first (with quadrant
// culling most staged entries still miss most pixels; no lane, no atomic), then a sum and a maximum over the lanes and the ballot's
// popcount, then ONE atomic per statistic per (wave, entry) from lane 0: float atomicAdd (weight_sum: the only output whose bits depend
// on the order the waves arrive in), atomicMax on the bit pattern of the non-negative float, integer atomicAdd.  The lane reduction is
// four DPP steps inside each row of 16 lanes (quad_perm xor 1, xor 2, row_half_mirror, row_mirror: operand modifiers of the add / max,
// no LDS traffic) and three scalar-operand adds of the four row totals (v_readlane); the other form tried, six __shfl_xor butterflies
// (ds_bpermute through the LDS crossbar), stays selectable for measurements (GSR_CONTRIB_REDUCE=1 in the environment) and gives the
// same bits: both add the same pairs in the same tree.  dominant_count needs no reduction: (best w, best id) per pixel in registers,
// one atomic per pixel at the end.
#include "common.hpp"
#include "render_walk.hpp"
#include "switches.hpp"
#include "tile_cull.hpp"

namespace gsr {

struct ContribArgs {
    const uint2* ranges;
    const uint32_t* tile_order;
    const uint32_t* point_list;
    const Splat* splat;
    int W, H, gridx, num_tiles, chunk_shift;
    uint32_t V;
    size_t g_stride, b_stride, iv_stride;
    const float* pixel_weights;   // [V][H][W] or NULL
    float* weight_sum;            // [P] or NULL
    uint32_t* weight_max;         // [P] or NULL: bit patterns of non-negative floats
    int* pixel_count;             // [P] or NULL
    int* dominant_count;          // [P] or NULL
};

constexpr int CS_ENTRY_WORDS = 8;   // x y A B | C o id -

template <int CTRL>
__device__ __forceinline__ float dpp_move(float v)
{
    return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), CTRL, 0xF, 0xF, true));
}

template <int LANE>
__device__ __forceinline__ float read_lane(float v)
{
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), LANE));
}

// sum and maximum of (s, m) over the wave's 64 lanes, valid in every lane; RED 0: DPP inside the rows + the four row totals through
// scalar registers, RED 1: shuffle butterflies.  Same tree of pairs in both.  m is non-negative (or NaN, which fmaxf drops).
template <int RED>
__device__ __forceinline__ void wave_sum_max(float& s, float& m)
{
    if constexpr (RED == 0) {
        s += dpp_move<0xB1>(s);  m = fmaxf(m, dpp_move<0xB1>(m));     // quad_perm [1 0 3 2]: lane ^ 1
        s += dpp_move<0x4E>(s);  m = fmaxf(m, dpp_move<0x4E>(m));     // quad_perm [2 3 0 1]: lane ^ 2
        s += dpp_move<0x141>(s); m = fmaxf(m, dpp_move<0x141>(m));    // row_half_mirror: the other quad of the 8
        s += dpp_move<0x140>(s); m = fmaxf(m, dpp_move<0x140>(m));    // row_mirror: the other 8 of the 16
        const float s0 = read_lane<0>(s), s1 = read_lane<16>(s), s2 = read_lane<32>(s), s3 = read_lane<48>(s);
        const float m0 = read_lane<0>(m), m1 = read_lane<16>(m), m2 = read_lane<32>(m), m3 = read_lane<48>(m);
        s = (s0 + s1) + (s2 + s3);
        m = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
    } else {
#pragma unroll
        for (int d = 1; d <= 32; d <<= 1) {   // (a float add is commutative bit for bit: both lanes of a pair get the same sum)
            s += __shfl_xor(s, d, 64);
            m = fmaxf(m, __shfl_xor(m, d, 64));
        }
    }
}

template <int RED>
__global__ __launch_bounds__(64) void k_contrib_stats(ContribArgs a)
{
    // the forward's work mapping (render_fwd.hip k_render_forward): the four quadrant waves of a tile on one XCD, views round-robin
    const uint32_t group = blockIdx.x >> 5;
    const uint32_t view = group % a.V;
    const uint32_t order_slot = (group / a.V) * 8u + (blockIdx.x & 7u);
    if (order_slot >= (uint32_t)a.num_tiles) return;
    a.ranges = at_view(a.ranges, a.iv_stride, view);
    a.tile_order = at_view(a.tile_order, a.iv_stride, view);
    a.point_list = at_view(a.point_list, a.b_stride, view);
    a.splat = at_view(a.splat, a.g_stride, view);
    const uint32_t tile = a.tile_order[order_slot];
    if (tile >= (uint32_t)a.num_tiles) return;   // (never: the forward wrote a permutation)
    const uint32_t q = (blockIdx.x >> 3) & 3u;
    const uint32_t lane = threadIdx.x;
    QuadGeom g;
    quad_geom(g, tile, q, a.gridx, a.W, a.H, lane);

    // the pixel's weight: !(m > 0) is 0, and 0 takes the pixel out of the walk
    float m = 1.f;
    if (a.pixel_weights != nullptr && g.inside) {
        const float v = a.pixel_weights[((size_t)view * (size_t)a.H + g.py) * (size_t)a.W + g.px];
        m = v > 0.f ? v : 0.f;
    }

    __shared__ __attribute__((aligned(16))) float stage[65 * CS_ENTRY_WORDS];   // 64 entries + one that may be read, never used

    const uint2 range = a.ranges[tile];
    const int total = (int)(range.y - range.x);

    float T = 1.0f;
    float best_w = 0.f;
    uint32_t best_id = 0;
    bool done = !g.inside || !(m > 0.f);
    bool all_done = __all(done);
    float bx0 = g.x0f, by0 = g.y0f, bx1 = g.x0f + 7.f, by1 = g.y0f + 7.f;
    if (!all_done) {
        int ax, ay, bx, by;
        live_box(__ballot(!done), ax, ay, bx, by);
        bx0 = g.x0f + (float)ax; by0 = g.y0f + (float)ay; bx1 = g.x0f + (float)bx; by1 = g.y0f + (float)by;
    }

    if (!all_done && total > 0) {
        const uint32_t* plist = a.point_list + range.x;
        // the forward's software pipeline: records of round r + 1 and ids of round r + 2 are in flight while round r is evaluated;
        // lanes past the end of the list read entry total - 1 again and are masked by `valid`
        const int last = total - 1;
        f32x4 c0, c1, n0, n1;
        uint32_t id_cur, id_nxt, id_nn;
        {
            prefetch4(id_cur, plist + ((int)lane < total ? (int)lane : last));
            prefetch4(id_nxt, plist + (64 + (int)lane < total ? 64 + (int)lane : last));
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(id_cur), "+v"(id_nxt)::"memory");
            const Splat* sp = a.splat + id_cur;
            prefetch16(c0, &sp->q0);
            prefetch16(c1, &sp->q1);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(c0), "+v"(c1)::"memory");
        }
        for (int base = 0; base < total; base += 64) {
            {
                const Splat* sp = a.splat + id_nxt;
                prefetch16(n0, &sp->q0);
                prefetch16(n1, &sp->q1);
                const int i2 = base + 128 + (int)lane;
                prefetch4(id_nn, plist + (i2 < total ? i2 : last));
            }
            const bool valid = base + (int)lane < total;
            const bool touch = valid && may_touch_rect(c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, bx0, by0, bx1, by1);
            const uint64_t mask = __ballot(touch);
            if (mask != 0) {
                const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                const int nsurv = (int)__popcll(mask);
                if (touch) {
                    float* p = stage + slot * CS_ENTRY_WORDS;
                    *(f32x4*)(p + 0) = c0;                                                        // x y A B
                    *(f32x4*)(p + 4) = f32x4{c1.x, c1.y, __uint_as_float(id_cur), 0.f};           // C o id
                }
                f32x4 ra = *(const f32x4*)(stage + 0), rb = *(const f32x4*)(stage + 4);
                for (int e = 0; e < nsurv; e++) {
                    const f32x4 e0 = ra, e1 = rb;
                    ra = *(const f32x4*)(stage + (e + 1) * CS_ENTRY_WORDS);      // the next entry, while this one is evaluated
                    rb = *(const f32x4*)(stage + (e + 1) * CS_ENTRY_WORDS + 4);
                    const uint32_t id = __builtin_amdgcn_readfirstlane(__float_as_uint(e1.z));
                    const float dx = e0.x - g.pixf_x, dy = e0.y - g.pixf_y;
                    const float power = power_exact(e0.z, e0.w, e1.x, dx, dy);
                    const float alpha = alpha_exact(e1.y, power);
                    const bool cnt = !done && !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
                    const float Tn = T * (1 - alpha);
                    const bool stop = cnt && (Tn < 0.0001f);
                    const bool hit = cnt && !stop;
                    const float w = hit ? alpha * T : 0.f;
                    T = hit ? Tn : T;
                    const uint64_t hits = __ballot(hit);
                    if (hits != 0) {
                        if (w > best_w) { best_w = w; best_id = id; }
                        float s = w * m, mx = s;   // (w = 0 where the entry missed the pixel)
                        wave_sum_max<RED>(s, mx);
                        if (lane == 0) {
                            if (a.weight_sum) atomicAdd(a.weight_sum + id, s);
                            if (a.weight_max) atomicMax(a.weight_max + id, __float_as_uint(mx));
                            if (a.pixel_count) atomicAdd(a.pixel_count + id, (int)__popcll(hits));
                        }
                    }
                    if (__any(stop)) {
                        done = done || stop;
                        const uint64_t live = __ballot(!done);
                        all_done = live == 0;
                        if (all_done) break;
                        int ax, ay, bx, by;   // a pixel stopped: the rounds still to come only need entries that reach the rest
                        live_box(live, ax, ay, bx, by);
                        bx0 = g.x0f + (float)ax; by0 = g.y0f + (float)ay; bx1 = g.x0f + (float)bx; by1 = g.y0f + (float)by;
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(n0), "+v"(n1), "+v"(id_nn)::"memory");
            if (all_done) break;
            c0 = n0; c1 = n1;
            id_cur = id_nxt;
            id_nxt = id_nn;
        }
    }

    if (a.dominant_count != nullptr && best_w > 0.f) atomicAdd(a.dominant_count + best_id, 1);
}

int launch_contrib_stats(const Launch& L, const gsr_params& p, const Batch& B, const uint32_t* point_list, const float* pixel_weights,
                         float* weight_sum, float* weight_max, int* pixel_count, int* dominant_count)
{
    ContribArgs a;
    a.ranges = B.iv.ranges;
    a.tile_order = B.iv.tile_order;
    a.point_list = point_list;
    a.splat = B.g.splat;
    set_frame_args(a, p, B);
    a.pixel_weights = pixel_weights;
    a.weight_sum = weight_sum;
    a.weight_max = reinterpret_cast<uint32_t*>(weight_max);
    a.pixel_count = pixel_count;
    a.dominant_count = dominant_count;
    const dim3 grid((unsigned)div_up(a.num_tiles, 8) * 32u * (unsigned)B.V);
    if (contrib_lane_reduce() == 1) hipLaunchKernelGGL(k_contrib_stats<1>, grid, dim3(64), 0, L.stream, a);
    else hipLaunchKernelGGL(k_contrib_stats<0>, grid, dim3(64), 0, L.stream, a);
    return check_launch(L, "contrib_stats");
}

}  // namespace gsr
