// view_stats.hip -- what a view batch's backward sums away: per-Gaussian density-control statistics over the V views and the per-view
// shares of dL/d mean2D, colour and opacity, from the gradient records a backward left in the arenas.
//
// k_preprocess_backward adds the records' words 0, 1 (mean2D), 5..7 (colour) and 8 (opacity) over the views, v = 0 .. V - 1, in
// float32 and hands out the sums.  This kernel reads the same records again, after any backward, and writes
//   grad_norm_sum[i]  = sum_v sqrt(gx_v^2 + gy_v^2)    every term and the running sum in float64 from the float32 words, views
//                                                      ascending, one rounding to float32 (an untouched record is an exact zero)
//   visible_views[i]  = #{v : radii[v][i] > 0}         max_radius[i] = max(0, max_v radii[v][i])
// -- overwriting, or (accumulate) added to / maxed with the caller's running values: float32(double(old) + sum), old + count,
// max(old, new) -- and, on request, the words themselves per view: [V][P][2], [V][P][3], [V][P], bit for bit, always overwritten.
// Adding those shares in float32 for v = 0, 1, .. reproduces the backward's summed outputs bit for bit (its loop starts from +0).
//
// One thread per Gaussian, the view loop inside the thread: every output row is written by exactly one thread, so there is nothing
// to add across threads -- no atomics, no scratch, and the result is a function of the records and radii alone.  Lane i reads 8 B
// (statistics) or 24 B (shares: words 0, 1 and 5..8) of record i, 64 B apart: every record is read once, nothing is reused, no
// workgroup remap.  The loads of four views are issued before the first is used (the V mod 4 views that remain are one shorter
// group); radii[v][i] and the [P] rows are coalesced as they are, a [V][P][2] row leaves as one 8-B store, a [V][P][3] row as one
// 12-B store.  Measured at 12 views x 800 K Gaussians: 0.130 ms (statistics, accumulate) / 0.160 ms (all outputs), 5.2 / 5.6 TB/s of
// lines and rows (profiles/r18_view_stats.txt).
#include "common.hpp"

namespace gsr {

constexpr int VS_THREADS = 256;
constexpr int VS_UNROLL = 4;     // views whose loads are in flight together

struct ViewStatsArgs {
    int P, V, accumulate;
    const int* radii;            // [V][P]
    const float* grad_rec;       // view 0's [P][GRAD_REC_WORDS]
    size_t gr_stride;
    float* grad_norm_sum;        // [P] or NULL
    int* visible_views;          // [P] or NULL
    int* max_radius;             // [P] or NULL
    float* mean2D_views;         // [V][P][2] or NULL (8-B aligned)
    float* color_views;          // [V][P][3] or NULL
    float* opacity_views;        // [V][P] or NULL
};

// N views of Gaussian i from view v0 on: every load is issued before the first value is used (one basic block: nothing for the
// compiler to sink a load into).  NORM: grad_norm_sum is wanted (words 0, 1 are read); SHARES: at least one per-view array is wanted
// (words 0, 1 and 5..8 are read).  Neither: the two integer statistics from radii alone.
template <bool NORM, bool SHARES, int N>
__device__ __forceinline__ void view_stats_group(const ViewStatsArgs& a, size_t i, int v0, double& sum, int& vis, int& rad)
{
    const size_t P = (size_t)a.P;
    float2 g[N];
    float4 c[N];     // words 4..7: x is the conic's third word, not handed out
    float op[N];
    int rd[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        rd[k] = a.radii[(size_t)(v0 + k) * P + i];
        if constexpr (NORM || SHARES) {
            const float* recp = at_view(a.grad_rec, a.gr_stride, (uint32_t)(v0 + k)) + i * GRAD_REC_WORDS;
            g[k] = *reinterpret_cast<const float2*>(recp);
            if constexpr (SHARES) {
                c[k] = *reinterpret_cast<const float4*>(recp + 4);
                op[k] = recp[8];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++) {
        vis += rd[k] > 0 ? 1 : 0;
        rad = rd[k] > rad ? rd[k] : rad;
        if constexpr (NORM) {
            const double gx = (double)g[k].x, gy = (double)g[k].y;
            sum += sqrt(gx * gx + gy * gy);
        }
        if constexpr (SHARES) {
            const size_t o = (size_t)(v0 + k) * P + i;
            if (a.mean2D_views) *reinterpret_cast<float2*>(a.mean2D_views + 2 * o) = g[k];
            if (a.color_views) {
                a.color_views[3 * o + 0] = c[k].y;
                a.color_views[3 * o + 1] = c[k].z;
                a.color_views[3 * o + 2] = c[k].w;
            }
            if (a.opacity_views) a.opacity_views[o] = op[k];
        }
    }
}

template <bool NORM, bool SHARES>
__global__ __launch_bounds__(VS_THREADS) void k_view_stats(ViewStatsArgs a)
{
    const int64_t row = (int64_t)blockIdx.x * VS_THREADS + threadIdx.x;
    if (row >= a.P) return;
    const size_t i = (size_t)row;

    // the caller's running values: asked for before the view loop, used after it
    const bool acc = a.accumulate != 0;
    const float old_sum = NORM && acc ? a.grad_norm_sum[i] : 0.f;
    const int old_vis = acc && a.visible_views ? a.visible_views[i] : 0;
    const int old_rad = acc && a.max_radius ? a.max_radius[i] : 0;

    double sum = 0.0;
    int vis = 0, rad = 0, v0 = 0;
    for (; v0 + VS_UNROLL <= a.V; v0 += VS_UNROLL) view_stats_group<NORM, SHARES, VS_UNROLL>(a, i, v0, sum, vis, rad);
    static_assert(VS_UNROLL == 4, "the remainder below is written for groups of four");
    switch (a.V - v0) {          // (uniform: V is a kernel argument)
    case 3: view_stats_group<NORM, SHARES, 3>(a, i, v0, sum, vis, rad); break;
    case 2: view_stats_group<NORM, SHARES, 2>(a, i, v0, sum, vis, rad); break;
    case 1: view_stats_group<NORM, SHARES, 1>(a, i, v0, sum, vis, rad); break;
    default: break;
    }
    if constexpr (NORM) a.grad_norm_sum[i] = acc ? (float)((double)old_sum + sum) : (float)sum;
    if (a.visible_views) a.visible_views[i] = old_vis + vis;
    if (a.max_radius) a.max_radius[i] = old_rad > rad ? old_rad : rad;
}

int launch_view_stats(const Launch& L, int P, const Batch& B, const int* radii, int accumulate, float* grad_norm_sum,
                      int* visible_views, int* max_radius, float* dL_dmean2D_views, float* dL_dcolor_views, float* dL_dopacity_views)
{
    ViewStatsArgs a;
    a.P = P; a.V = B.V; a.accumulate = accumulate;
    a.radii = radii; a.grad_rec = B.grad_rec; a.gr_stride = B.gr_stride;
    a.grad_norm_sum = grad_norm_sum; a.visible_views = visible_views; a.max_radius = max_radius;
    a.mean2D_views = dL_dmean2D_views; a.color_views = dL_dcolor_views; a.opacity_views = dL_dopacity_views;
    const dim3 grid((unsigned)div_up(P, VS_THREADS)), block(VS_THREADS);
    const bool norm = grad_norm_sum != nullptr, shares = dL_dmean2D_views || dL_dcolor_views || dL_dopacity_views;
    if (norm && shares) hipLaunchKernelGGL((k_view_stats<true, true>), grid, block, 0, L.stream, a);
    else if (norm) hipLaunchKernelGGL((k_view_stats<true, false>), grid, block, 0, L.stream, a);
    else if (shares) hipLaunchKernelGGL((k_view_stats<false, true>), grid, block, 0, L.stream, a);
    else hipLaunchKernelGGL((k_view_stats<false, false>), grid, block, 0, L.stream, a);
    return check_launch(L, "view_stats");
}

}  // namespace gsr
