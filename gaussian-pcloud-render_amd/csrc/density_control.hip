// density_control.hip -- adaptive density control: clone, split and prune in one pass (include/gsr.h
// gsr_density_plan, gsr_density_apply, which state the definition formula by formula).
//
// The plan, three launches, no atomics and no look-back:
//   k_density_decide    one lane per Gaussian: the action code (28 B read, 1 B written), and per workgroup the counts of rows, carried
//                       rows, copies and vanished Gaussians from two packed workgroup scans.
//   k_density_scan      ONE workgroup turns the row counts into exclusive bases in place, DENSITY_SCAN_ROUND of them per round of its
//                       loop with a running carry, sums the other three counts in 64 bits, and writes totals and offsets[P].
//   k_density_offsets   one lane per Gaussian again: rows of the action code, a workgroup scan, plus the workgroup's base.
// The apply, one or two launches:
//   k_density_index     one lane per source Gaussian writes its 0..2 entries of the output-row -> source map (only when the caller
//                       wants `index`; without it the gather finds a row's source by bisection of `offsets`).
//   k_density_gather    ONE launch for the 1..8 groups of the call, output-driven: lanes run over the flat [P_out * width] output of
//                       their group (the group table travels by value; a workgroup finds its group from the prefix of block counts), so
//                       stores are contiguous, and because sources ascend with the output rows the loads are contiguous within a source
//                       row's run.  16 B per lane where a group's pointers and width allow it, element by element otherwise.  A child's
//                       noise and rotation are evaluated by the three lanes that write its mean.
//
// Built with -ffp-contract=off: one rounding per written operation; division and square root are the correctly rounded ones.
#include "density_control.hpp"

#include "block_scan.hpp"
#include "host.hpp"
#include "splat_math.hpp"

namespace gsr {

__device__ __forceinline__ uint32_t action_rows(uint32_t a)
{
    return a == GSR_DENSITY_CLONED || a == GSR_DENSITY_SPLIT ? 2u : a == GSR_DENSITY_PRUNED ? 0u : 1u;
}

// the definition of include/gsr.h, in its order
__device__ __forceinline__ uint32_t decide(const DensityRuleDev& r, float sx, float sy, float sz, float opacity, float grad_sum, int views,
                                           int radius, bool masked)
{
    if (r.log_scales) {
        sx = expf(sx);
        sy = expf(sy);
        sz = expf(sz);
    }
    const float smax = fmax_(fmax_(sx, sy), sz);
    const float g = grad_sum / (float)(views > 1 ? views : 1);
    const bool hot = g >= r.grad_threshold;
    const bool dead = opacity < r.min_opacity || masked;
    const bool big = (r.max_screen_radius > 0 && radius > r.max_screen_radius) || (r.max_world_size > 0.f && smax > r.max_world_size);
    if (hot && smax <= r.dense_size) return dead ? GSR_DENSITY_PRUNED : big ? GSR_DENSITY_CLONED_COPY : GSR_DENSITY_CLONED;
    if (hot && smax > r.dense_size)
        return dead || (r.max_world_size > 0.f && smax / 1.6f > r.max_world_size) ? GSR_DENSITY_PRUNED : GSR_DENSITY_SPLIT;
    return dead || big ? GSR_DENSITY_PRUNED : GSR_DENSITY_KEPT;
}

__global__ __launch_bounds__(DENSITY_THREADS) void k_density_decide(DensityRuleDev r, DensityPlanArgs a, uint32_t nblk)
{
    __shared__ uint32_t tmp[4];
    const uint32_t i = blockIdx.x * DENSITY_THREADS + threadIdx.x;
    uint32_t rows = 0, carried = 0, copies = 0, gone = 0;
    if (i < (uint32_t)a.P) {
        const float* s = a.scales + (size_t)i * 3;
        const uint32_t act = decide(r, s[0], s[1], s[2], a.opacities[i], a.grad_norm_sum[i], a.visible_views[i], a.max_radius[i],
                                    a.prune_mask != nullptr && a.prune_mask[i] != 0);
        a.action[i] = (uint8_t)act;
        rows = action_rows(act);
        carried = act == GSR_DENSITY_KEPT || act == GSR_DENSITY_CLONED;
        copies = act == GSR_DENSITY_CLONED || act == GSR_DENSITY_CLONED_COPY;
        gone = act == GSR_DENSITY_PRUNED;
    }
    // every count of a workgroup is at most 512: two of them share a word
    uint32_t t0, t1;
    block_exclusive_scan_256(rows | carried << 16, tmp, &t0);
    block_exclusive_scan_256(copies | gone << 16, tmp, &t1);
    if (threadIdx.x == 0) {
        a.counts[blockIdx.x] = t0 & 0xFFFFu;
        a.counts[nblk + blockIdx.x] = t0 >> 16;
        a.counts[2 * (size_t)nblk + blockIdx.x] = t1 & 0xFFFFu;
        a.counts[3 * (size_t)nblk + blockIdx.x] = t1 >> 16;
    }
}

__global__ __launch_bounds__(DENSITY_THREADS) void k_density_scan(DensityPlanArgs a, uint32_t nblk)
{
    __shared__ uint32_t tmp[4];
    __shared__ unsigned long long sums[3][DENSITY_THREADS];
    uint32_t carry = 0;
    unsigned long long mine[3] = {0ull, 0ull, 0ull};
    for (uint32_t base = 0; base < nblk; base += DENSITY_SCAN_ROUND) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < nblk ? a.counts[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan_256(v, tmp, &total);
        if (b < nblk) {
            a.counts[b] = carry + ex;
#pragma unroll
            for (int k = 0; k < 3; k++) mine[k] += a.counts[(size_t)(k + 1) * nblk + b];
        }
        carry += total;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) sums[k][threadIdx.x] = mine[k];
    __syncthreads();
    for (uint32_t s = DENSITY_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < 3; k++) sums[k][threadIdx.x] += sums[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long long rows = (long long)carry, carried = (long long)sums[0][0], copies = (long long)sums[1][0];
        a.offsets[a.P] = carry;
        a.totals[0] = rows;
        a.totals[1] = carried;
        a.totals[2] = copies;
        a.totals[3] = rows - carried - copies;   // children
        a.totals[4] = (long long)sums[2][0];
    }
}

__global__ __launch_bounds__(DENSITY_THREADS) void k_density_offsets(DensityPlanArgs a)
{
    __shared__ uint32_t tmp[4];
    const uint32_t i = blockIdx.x * DENSITY_THREADS + threadIdx.x;
    const uint32_t rows = i < (uint32_t)a.P ? action_rows(a.action[i]) : 0u;
    const uint32_t ex = block_exclusive_scan_256(rows, tmp, nullptr);
    if (i < (uint32_t)a.P) a.offsets[i] = a.counts[blockIdx.x] + ex;
}

__global__ __launch_bounds__(DENSITY_THREADS) void k_density_index(DensityApplyArgs a)
{
    const uint32_t i = blockIdx.x * DENSITY_THREADS + threadIdx.x;
    if (i >= (uint32_t)a.P) return;
    const uint32_t act = a.action[i], o = a.offsets[i];
    const int32_t carried = (int32_t)i, fresh = -1 - (int32_t)i;
    const uint32_t rows = action_rows(act);
    if (rows >= 1 && o < a.P_out) a.index[o] = act == GSR_DENSITY_KEPT || act == GSR_DENSITY_CLONED ? carried : fresh;
    if (rows == 2 && o + 1 < a.P_out) a.index[o + 1] = fresh;
}

// ---- the noise of a child: Philox4x32-10 on (i, k, 0, 0), Box-Muller in float32 (include/gsr.h) ----
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

__device__ __forceinline__ void child_noise(const DensityRuleDev& r, uint32_t i, uint32_t k, float eps[3])
{
    uint32_t x[4];
    philox4x32_10(i, k, 0u, 0u, r.key0, r.key1, x);
    float u[4];
#pragma unroll
    for (int j = 0; j < 4; j++) u[j] = ((float)(x[j] >> 8) + 0.5f) * 0x1p-24f;
    const float two_pi = 6.2831855f;
    const float r01 = sqrtf(-2.0f * logf(u[0]));
    eps[0] = r01 * cosf(two_pi * u[1]);
    eps[1] = r01 * sinf(two_pi * u[1]);
    eps[2] = sqrtf(-2.0f * logf(u[2])) * cosf(two_pi * u[3]);
}

// component `row` of the mean of child k of parent i, whose mean component is mu
__device__ __forceinline__ float child_mean(const DensityRuleDev& r, const DensityApplyArgs& a, uint32_t i, uint32_t k, uint32_t row, float mu)
{
    const float* s = a.scales + (size_t)i * 3;
    float sx = s[0], sy = s[1], sz = s[2];
    if (r.log_scales) {
        sx = expf(sx);
        sy = expf(sy);
        sz = expf(sz);
    }
    const float* q = a.rotations + (size_t)i * 4;
    float qr = q[0], qx = q[1], qy = q[2], qz = q[3];
    if (r.normalize_rotations) {
        const float n = sqrtf(((qr * qr + qx * qx) + qy * qy) + qz * qz);
        qr = qr / n;
        qx = qx / n;
        qy = qy / n;
        qz = qz / n;
    }
    const M3 R = quat_to_cols(qr, qx, qy, qz);   // R.m[row] is row `row` of the rotation (the argument triples)
    float eps[3];
    if (a.noise != nullptr) {
        const float* e = a.noise + ((size_t)i * 2 + k) * 3;
        eps[0] = e[0];
        eps[1] = e[1];
        eps[2] = e[2];
    } else {
        child_noise(r, i, k, eps);
    }
    const float t0 = sx * eps[0], t1 = sy * eps[1], t2 = sz * eps[2];
    const float r0 = row == 0 ? R.m[0][0] : row == 1 ? R.m[1][0] : R.m[2][0];
    const float r1 = row == 0 ? R.m[0][1] : row == 1 ? R.m[1][1] : R.m[2][1];
    const float r2 = row == 0 ? R.m[0][2] : row == 1 ? R.m[1][2] : R.m[2][2];
    const float d = (r0 * t0 + r1 * t1) + r2 * t2;
    return mu + d;
}

// Output row j: its source Gaussian, and whether the row is new (a copy or a child).  false: no such source (a P_out beyond the plan's,
// or a plan that is not one) -- nothing is stored for the row.
template <bool HAS_INDEX>
__device__ __forceinline__ bool row_source(const DensityApplyArgs& a, uint32_t j, uint32_t& src, bool& fresh)
{
    if (HAS_INDEX) {
        const int32_t s = a.index[j];
        fresh = s < 0;
        src = (uint32_t)(fresh ? -1 - s : s);
        return src < (uint32_t)a.P;
    }
    // the last i with offsets[i] <= j: Gaussians without rows share their successor's offset and are stepped over
    uint32_t lo = 0, hi = (uint32_t)a.P;   // offsets[lo] <= j (offsets[0] = 0), the answer is below hi
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.offsets[mid] <= j) lo = mid; else hi = mid;
    }
    src = lo;
    const uint32_t act = a.action[src], k = j - a.offsets[src];
    fresh = !(act == GSR_DENSITY_KEPT || (act == GSR_DENSITY_CLONED && k == 0));
    return k < action_rows(act);
}

template <bool HAS_INDEX>
__device__ __forceinline__ void gather_scalar(const DensityRuleDev& r, const DensityGroupDev& g, const DensityApplyArgs& a, uint32_t e)
{
    const uint32_t j = e / g.width, col = e - j * g.width;
    uint32_t src;
    bool fresh;
    if (!row_source<HAS_INDEX>(a, j, src, fresh)) return;
    float v = g.src[(size_t)src * g.width + col];
    if (g.role == GSR_DENSITY_MOMENT) {
        if (fresh) v = 0.f;
    } else if (g.role != GSR_DENSITY_COPY && a.action[src] == GSR_DENSITY_SPLIT) {
        if (g.role == GSR_DENSITY_SCALES) {
            v = r.log_scales ? v - 0x1.e148a2p-2f : v / 1.6f;
        } else {
            const uint32_t k = j - a.offsets[src];
            if (k > 1u) return;   // (an index that is not this plan's: the noise has two children per parent)
            v = child_mean(r, a, src, k, col, v);
        }
    }
    g.dst[e] = v;
}

template <bool HAS_INDEX>
__global__ __launch_bounds__(DENSITY_THREADS) void k_density_gather(DensityRuleDev r, DensityTable t, DensityApplyArgs a)
{
    // this workgroup's group: static indices into the by-value table, selected by a workgroup-uniform comparison
    DensityGroupDev g = t.g[0];
    uint32_t first = 0;
#pragma unroll
    for (int k = 1; k < DENSITY_MAX_GROUPS; k++) {
        if (k < t.G && blockIdx.x >= t.g[k - 1].block_end) {
            g = t.g[k];
            first = t.g[k - 1].block_end;
        }
    }
    const size_t block = blockIdx.x - first, nblocks = g.block_end - first;
    const size_t n = g.n;

    if (!g.vec) {
        for (size_t base = block * DENSITY_BLOCK_ELEMS; base < n; base += nblocks * DENSITY_BLOCK_ELEMS) {
#pragma unroll
            for (int k = 0; k < DENSITY_VEC; k++) {
                const size_t e = base + (size_t)k * DENSITY_THREADS + threadIdx.x;
                if (e < n) gather_scalar<HAS_INDEX>(r, g, a, (uint32_t)e);
            }
        }
        return;
    }
    // width % 4 == 0: a 4-vector lies inside one row, n % 4 == 0, and rows of src and dst start on 16-B boundaries
    const size_t nvec = n / DENSITY_VEC;
    float4* const D4 = reinterpret_cast<float4*>(g.dst);
    for (size_t i = block * DENSITY_THREADS + threadIdx.x; i < nvec; i += nblocks * DENSITY_THREADS) {
        const uint32_t e = (uint32_t)i * DENSITY_VEC, j = e / g.width, col = e - j * g.width;
        uint32_t src;
        bool fresh;
        if (!row_source<HAS_INDEX>(a, j, src, fresh)) continue;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!(g.role == GSR_DENSITY_MOMENT && fresh)) v = *reinterpret_cast<const float4*>(g.src + (size_t)src * g.width + col);
        D4[i] = v;
    }
}

int launch_density_plan(const Launch& L, const DensityRuleDev& r, const DensityPlanArgs& a)
{
    const uint32_t nblk = (uint32_t)density_blocks(a.P);
    hipLaunchKernelGGL(k_density_decide, dim3(nblk), dim3(DENSITY_THREADS), 0, L.stream, r, a, nblk);
    hipLaunchKernelGGL(k_density_scan, dim3(1), dim3(DENSITY_THREADS), 0, L.stream, a, nblk);
    hipLaunchKernelGGL(k_density_offsets, dim3(nblk), dim3(DENSITY_THREADS), 0, L.stream, a);
    return check_launch(L, "density_plan");
}

int launch_density_apply(const Launch& L, const DensityRuleDev& r, const DensityTable& t, const DensityApplyArgs& a)
{
    if (a.index != nullptr) {
        hipLaunchKernelGGL(k_density_index, dim3((uint32_t)density_blocks(a.P)), dim3(DENSITY_THREADS), 0, L.stream, a);
        hipLaunchKernelGGL(k_density_gather<true>, dim3(t.g[t.G - 1].block_end), dim3(DENSITY_THREADS), 0, L.stream, r, t, a);
    } else {
        hipLaunchKernelGGL(k_density_gather<false>, dim3(t.g[t.G - 1].block_end), dim3(DENSITY_THREADS), 0, L.stream, r, t, a);
    }
    return check_launch(L, "density_apply");
}

}  // namespace gsr
