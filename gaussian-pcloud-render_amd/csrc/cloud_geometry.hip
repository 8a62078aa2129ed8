// cloud_geometry.hip -- point-cloud neighbourhoods: exact k nearest neighbours, spacing, PCA normals and orientations (DESIGN.md
// section 4k; include/gsr.h gsr_knn, gsr_cloud_geometry, which state the definition formula by formula).
//
// gsr_knn, six launches and the library's radix sort, no atomics, no look-back, nothing read back:
//   k_cloud_bounds_part  per-workgroup min/max of the present points and their count (grid-stride, at most CLOUD_MAX_PARTS workgroups)
//   k_cloud_bounds       ONE workgroup folds the parts into the cloud's box and the number of present points
//   k_cloud_keys         one lane per point: a 30-bit Morton key inside that box, absent points keyed behind every present one
//   (launch_radix_sort_pairs: 31 key bits, iota values)
//   k_cloud_gather       one lane per sorted position: (x, y, z, index) as one 16-B record, and one tight box per run of 64 (a wave)
//   k_cloud_coarse       one wave per 64 runs: their boxes' box
//   k_knn_search<KMAX>   one wave per run answers its 64 queries.  Each lane keeps its sorted list of KMAX >= K entries in registers;
//                        a candidate run is loaded once, one record per lane, and handed round by v_readlane.  The walk: the own run,
//                        the runs of the own coarse box, then every other coarse box and -- inside a surviving one -- its runs.  A box
//                        is skipped only when every lane's bound is strictly greater than its K-th distance.
// The order in which candidates arrive cannot show: the K smallest of a strict total order (d2, index) are one set.
// gsr_cloud_geometry: k_cloud_geometry, one lane per point.
//
// Built with -ffp-contract=off: one rounding per written operation; division and square root are the correctly rounded ones.
#include "cloud_geometry.hpp"

#include <cmath>

#include "host.hpp"

namespace gsr {

namespace {

constexpr float INF = __builtin_huge_valf();
constexpr int NO_INDEX = 0x7FFFFFFF;   // a list slot that holds no neighbour: behind every index at d2 = +inf; stored as -1

__device__ __forceinline__ float min_(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float max_(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min_(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max_(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

struct Box {
    float lo[3], hi[3];
};
__device__ __forceinline__ Box empty_box()
{
    Box b;
#pragma unroll
    for (int a = 0; a < 3; a++) { b.lo[a] = INF; b.hi[a] = -INF; }
    return b;
}
__device__ __forceinline__ void box_add(Box& b, float x, float y, float z)
{
    b.lo[0] = min_(b.lo[0], x); b.hi[0] = max_(b.hi[0], x);
    b.lo[1] = min_(b.lo[1], y); b.hi[1] = max_(b.hi[1], y);
    b.lo[2] = min_(b.lo[2], z); b.hi[2] = max_(b.hi[2], z);
}
__device__ __forceinline__ void box_merge(Box& b, const float* w)
{
#pragma unroll
    for (int a = 0; a < 3; a++) { b.lo[a] = min_(b.lo[a], w[a]); b.hi[a] = max_(b.hi[a], w[3 + a]); }
}
__device__ __forceinline__ Box wave_box(Box b)
{
#pragma unroll
    for (int a = 0; a < 3; a++) { b.lo[a] = wave_min(b.lo[a]); b.hi[a] = wave_max(b.hi[a]); }
    return b;
}
__device__ __forceinline__ void box_store(float* w, const Box& b, uint32_t count)
{
#pragma unroll
    for (int a = 0; a < 3; a++) { w[a] = b.lo[a]; w[3 + a] = b.hi[a]; }
    w[6] = __uint_as_float(count);
    w[7] = 0.f;
}

// the workgroup's box and count from its CLOUD_THREADS lanes'; valid in thread 0
__device__ __forceinline__ void block_box(Box& b, uint32_t& n, float (*red)[CLOUD_BOX_WORDS])
{
    b = wave_box(b);
    n = wave_sum(n);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) box_store(red[w], b, n);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < CLOUD_THREADS / 64; k++) {
            box_merge(b, red[k]);
            n += __float_as_uint(red[k][6]);
        }
    }
}

__global__ __launch_bounds__(CLOUD_THREADS) void k_cloud_bounds_part(int P, const float* __restrict__ points, float* __restrict__ parts)
{
    __shared__ float red[CLOUD_THREADS / 64][CLOUD_BOX_WORDS];
    Box b = empty_box();
    uint32_t n = 0;
    for (size_t i = (size_t)blockIdx.x * CLOUD_THREADS + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * CLOUD_THREADS) {
        const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
        if (finite3(x, y, z)) {
            box_add(b, x, y, z);
            n++;
        }
    }
    block_box(b, n, red);
    if (threadIdx.x == 0) box_store(parts + (size_t)blockIdx.x * CLOUD_BOX_WORDS, b, n);
}

__global__ __launch_bounds__(CLOUD_THREADS) void k_cloud_bounds(int nparts, const float* __restrict__ parts, float* __restrict__ box)
{
    __shared__ float red[CLOUD_THREADS / 64][CLOUD_BOX_WORDS];
    Box b = empty_box();
    uint32_t n = 0;
    for (int k = threadIdx.x; k < nparts; k += CLOUD_THREADS) {
        box_merge(b, parts + (size_t)k * CLOUD_BOX_WORDS);
        n += __float_as_uint(parts[(size_t)k * CLOUD_BOX_WORDS + 6]);
    }
    block_box(b, n, red);
    if (threadIdx.x == 0) box_store(box, b, n);
}

// bits 0..9 of v spread to every third bit
__device__ __forceinline__ uint32_t spread3(uint32_t v)
{
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// the cell of coordinate q on an axis [lo, hi] cut into 1024: any value in 0..1023 is a valid answer (the key orders the walk, it does
// not enter the result), so a flat or overflowing axis simply yields cell 0
__device__ __forceinline__ uint32_t cell(float q, float lo, float hi)
{
    const float ext = hi - lo;
    const float inv = (ext > 0.f && isfinite(ext)) ? 1024.f / ext : 0.f;
    const float t = (q - lo) * inv;
    return (uint32_t)(int)min_(max_(t == t ? t : 0.f, 0.f), 1023.f);
}

__global__ __launch_bounds__(CLOUD_THREADS) void k_cloud_keys(int P, const float* __restrict__ points, const float* __restrict__ box,
                                                              uint32_t* __restrict__ keys)
{
    const size_t i = (size_t)blockIdx.x * CLOUD_THREADS + threadIdx.x;
    if (i >= (size_t)P) return;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    uint32_t key = CLOUD_ABSENT_KEY;
    if (finite3(x, y, z)) key = spread3(cell(x, box[0], box[3])) | spread3(cell(y, box[1], box[4])) << 1 | spread3(cell(z, box[2], box[5])) << 2;
    keys[i] = key;
}

__global__ __launch_bounds__(CLOUD_THREADS) void k_cloud_gather(int P, const float* __restrict__ points, const uint32_t* __restrict__ order,
                                                                float4* __restrict__ sorted, float* __restrict__ fine)
{
    const size_t pos = (size_t)blockIdx.x * CLOUD_THREADS + threadIdx.x;
    Box b = empty_box();
    if (pos < (size_t)P) {
        const uint32_t j = order[pos];
        float x = 0.f, y = 0.f, z = 0.f;
        if (j < (uint32_t)P) {   // (always: the sort permutes 0..P-1)
            x = points[3 * (size_t)j];
            y = points[3 * (size_t)j + 1];
            z = points[3 * (size_t)j + 2];
        }
        sorted[pos] = make_float4(x, y, z, __uint_as_float(j));
        if (finite3(x, y, z)) box_add(b, x, y, z);
    }
    b = wave_box(b);
    const size_t run = pos >> 6;   // the wave's
    if ((threadIdx.x & 63) == 0 && run < ((size_t)P + CLOUD_RUN - 1) / CLOUD_RUN) box_store(fine + run * CLOUD_BOX_WORDS, b, 0u);
}

__global__ __launch_bounds__(CLOUD_THREADS) void k_cloud_coarse(int nruns, int ncoarse, const float* __restrict__ fine, float* __restrict__ coarse)
{
    const int c = blockIdx.x * (CLOUD_THREADS / 64) + (threadIdx.x >> 6);   // wave-uniform
    const int f = c * CLOUD_COARSE + (threadIdx.x & 63);
    Box b = empty_box();
    if (c < ncoarse && f < nruns) box_merge(b, fine + (size_t)f * CLOUD_BOX_WORDS);
    b = wave_box(b);
    if (c < ncoarse && (threadIdx.x & 63) == 0) box_store(coarse + (size_t)c * CLOUD_BOX_WORDS, b, 0u);
}

// ---- the search -----------------------------------------------------------------------------------------------------------------
template <int KMAX>
struct KnnList {
    float d[KMAX];
    int id[KMAX];
    float kth_d;   // entry K - 1, the one a candidate has to beat
    int kth_id;
};

__device__ __forceinline__ bool before(float da, int ja, float db, int jb) { return da < db || (da == db && ja < jb); }

template <int KMAX>
__device__ __forceinline__ void knn_insert(KnnList<KMAX>& l, int K, float dc, int jc)
{
#pragma unroll
    for (int s = KMAX - 1; s > 0; s--) {
        const bool lt_prev = before(dc, jc, l.d[s - 1], l.id[s - 1]);
        const bool lt_cur = before(dc, jc, l.d[s], l.id[s]);
        l.d[s] = lt_prev ? l.d[s - 1] : lt_cur ? dc : l.d[s];
        l.id[s] = lt_prev ? l.id[s - 1] : lt_cur ? jc : l.id[s];
    }
    if (before(dc, jc, l.d[0], l.id[0])) {
        l.d[0] = dc;
        l.id[0] = jc;
    }
#pragma unroll
    for (int s = 0; s < KMAX; s++) {
        if (s == K - 1) {
            l.kth_d = l.d[s];
            l.kth_id = l.id[s];
        }
    }
}

// the float32 lower bound of d2 between q and any point of the box (include/gsr.h: the same written operations as d2)
__device__ __forceinline__ float box_bound(const float* __restrict__ w, float qx, float qy, float qz)
{
    const float gx = max_(max_(w[0] - qx, qx - w[3]), 0.f);
    const float gy = max_(max_(w[1] - qy, qy - w[4]), 0.f);
    const float gz = max_(max_(w[2] - qz, qz - w[5]), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

// the candidates of run f (its first `cnt` sorted positions) against every lane's query
template <int KMAX>
__device__ __forceinline__ void knn_visit(KnnList<KMAX>& l, int K, const float4* __restrict__ sorted, uint32_t f, uint32_t cnt, bool valid,
                                          uint32_t pos, float qx, float qy, float qz)
{
    const uint32_t lane = threadIdx.x & 63;
    const float4 c = lane < cnt ? sorted[(size_t)f * CLOUD_RUN + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t s = 0; s < cnt; s++) {
        const float cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.x), (int)s));
        const float cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.y), (int)s));
        const float cz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.z), (int)s));
        const int cj = __builtin_amdgcn_readlane(__float_as_int(c.w), (int)s);
        const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (valid && f * CLOUD_RUN + s != pos && before(d2, cj, l.kth_d, l.kth_id)) knn_insert<KMAX>(l, K, d2, cj);
    }
}

template <int KMAX>
__global__ __launch_bounds__(64) void k_knn_search(int P, int K, const float4* __restrict__ sorted, const float* __restrict__ box,
                                                   const float* __restrict__ fine, const float* __restrict__ coarse,
                                                   int32_t* __restrict__ idx, float* __restrict__ d2_out)
{
    const uint32_t n_present = min(__float_as_uint(box[6]), (uint32_t)P);
    const uint32_t nf = (n_present + CLOUD_RUN - 1) / CLOUD_RUN, nc = (nf + CLOUD_COARSE - 1) / CLOUD_COARSE;
    const uint32_t run = blockIdx.x, own_coarse = run / CLOUD_COARSE;
    const uint32_t pos = run * CLOUD_RUN + threadIdx.x;
    const bool valid = pos < n_present;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pos < (uint32_t)P) q = sorted[pos];

    KnnList<KMAX> l;
#pragma unroll
    for (int s = 0; s < KMAX; s++) {
        l.d[s] = INF;
        l.id[s] = NO_INDEX;
    }
    l.kth_d = INF;
    l.kth_id = NO_INDEX;

    const auto cnt_of = [n_present](uint32_t f) { return min((uint32_t)CLOUD_RUN, n_present - f * CLOUD_RUN); };
    if (run < nf) {   // (a run of absent points alone has no query)
        knn_visit<KMAX>(l, K, sorted, run, cnt_of(run), valid, pos, q.x, q.y, q.z);
        // the runs of the own coarse box, then the other coarse boxes: every box at most once
        for (uint32_t f = own_coarse * CLOUD_COARSE; f < min(nf, (own_coarse + 1) * CLOUD_COARSE); f++) {
            if (f == run) continue;
            const bool want = valid && !(box_bound(fine + (size_t)f * CLOUD_BOX_WORDS, q.x, q.y, q.z) > l.kth_d);
            if (__any(want)) knn_visit<KMAX>(l, K, sorted, f, cnt_of(f), valid, pos, q.x, q.y, q.z);
        }
        for (uint32_t c = 0; c < nc; c++) {
            if (c == own_coarse) continue;
            const bool near = valid && !(box_bound(coarse + (size_t)c * CLOUD_BOX_WORDS, q.x, q.y, q.z) > l.kth_d);
            if (!__any(near)) continue;
            for (uint32_t f = c * CLOUD_COARSE; f < min(nf, (c + 1) * CLOUD_COARSE); f++) {
                const bool want = valid && !(box_bound(fine + (size_t)f * CLOUD_BOX_WORDS, q.x, q.y, q.z) > l.kth_d);
                if (__any(want)) knn_visit<KMAX>(l, K, sorted, f, cnt_of(f), valid, pos, q.x, q.y, q.z);
            }
        }
    }
    if (pos >= (uint32_t)P) return;
    const uint32_t me = __float_as_uint(q.w);
    if (me >= (uint32_t)P) return;   // (never: the sort permutes 0..P-1)
    int32_t* const row = idx + (size_t)me * K;
    float* const drow = d2_out ? d2_out + (size_t)me * K : nullptr;
#pragma unroll
    for (int s = 0; s < KMAX; s++) {
        if (s < K) {
            row[s] = l.id[s] == NO_INDEX ? -1 : l.id[s];
            if (drow) drow[s] = l.d[s];
        }
    }
}

// ---- per-point geometry ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void jacobi_rotate(float A[3][3], float V[3][3], int p, int q, int r)
{
    const float apq = A[p][q];
    if (apq == 0.f) return;
    const float theta = (A[q][q] - A[p][p]) / (2.f * apq);
    const float sgn = theta >= 0.f ? 1.f : -1.f;
    const float t = sgn / (fabsf(theta) + sqrtf(theta * theta + 1.f));
    const float c = 1.f / sqrtf(t * t + 1.f);
    const float s = t * c;
    const float h = t * apq;
    A[p][p] = A[p][p] - h;
    A[q][q] = A[q][q] + h;
    A[p][q] = A[q][p] = 0.f;
    const float arp = A[r][p], arq = A[r][q];
    A[r][p] = A[p][r] = c * arp - s * arq;
    A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

__device__ __forceinline__ void order_pair(float lam[3], float V[3][3], int i, int j)
{
    if (lam[i] > lam[j]) {
        const float t = lam[i];
        lam[i] = lam[j];
        lam[j] = t;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float v = V[k][i];
            V[k][i] = V[k][j];
            V[k][j] = v;
        }
    }
}

__global__ __launch_bounds__(CLOUD_THREADS) void k_cloud_geometry(CloudGeometryArgs a)
{
    const size_t i = (size_t)blockIdx.x * CLOUD_THREADS + threadIdx.x;
    if (i >= (size_t)a.P) return;
    const float px = a.points[3 * i], py = a.points[3 * i + 1], pz = a.points[3 * i + 2];
    const bool self_ok = finite3(px, py, pz);
    const int32_t* const row = a.knn_idx + i * (size_t)a.K;

    // pass 1: the spacing sum over the first k_s present entries, the delta sum over the first k_n
    float ssum = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    int present = 0;
    for (int k = 0; k < a.K && self_ok; k++) {
        const int32_t j = row[k];
        if (j < 0 || j >= a.P) continue;
        const float x = a.points[3 * (size_t)j], y = a.points[3 * (size_t)j + 1], z = a.points[3 * (size_t)j + 2];
        if (!finite3(x, y, z)) continue;
        const float dx = x - px, dy = y - py, dz = z - pz;
        if (present < a.k_s) ssum = ssum + ((dx * dx + dy * dy) + dz * dz);
        if (present < a.k_n) {
            sx = sx + dx;
            sy = sy + dy;
            sz = sz + dz;
        }
        present++;
    }
    const int n_s = present < a.k_s ? present : a.k_s, n_n = present < a.k_n ? present : a.k_n;
    if (a.spacing) a.spacing[i] = n_s > 0 ? sqrtf(ssum / (float)n_s) : 0.f;
    if (!a.cov6 && !a.eigenvalues && !a.normals && !a.rotations) return;

    float C[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float lam[3] = {0.f, 0.f, 0.f};
    float n[3] = {0.f, 0.f, 1.f};
    float quat[4] = {1.f, 0.f, 0.f, 0.f};
    if (n_n >= 2) {
        const float fn = (float)(n_n + 1);
        const float mx = sx / fn, my = sy / fn, mz = sz / fn;
        // pass 2: the scatter about the mean, the point itself first
        float ex = 0.f - mx, ey = 0.f - my, ez = 0.f - mz;
        float xx = ex * ex, xy = ex * ey, xz = ex * ez, yy = ey * ey, yz = ey * ez, zz = ez * ez;
        int seen = 0;
        for (int k = 0; k < a.K && seen < n_n; k++) {
            const int32_t j = row[k];
            if (j < 0 || j >= a.P) continue;
            const float x = a.points[3 * (size_t)j], y = a.points[3 * (size_t)j + 1], z = a.points[3 * (size_t)j + 2];
            if (!finite3(x, y, z)) continue;
            const float dx = x - px, dy = y - py, dz = z - pz;
            ex = dx - mx;
            ey = dy - my;
            ez = dz - mz;
            xx = xx + ex * ex;
            xy = xy + ex * ey;
            xz = xz + ex * ez;
            yy = yy + ey * ey;
            yz = yz + ey * ez;
            zz = zz + ez * ez;
            seen++;
        }
        C[0] = xx / fn; C[1] = xy / fn; C[2] = xz / fn; C[3] = yy / fn; C[4] = yz / fn; C[5] = zz / fn;

        if (a.eigenvalues || a.normals || a.rotations) {
            float A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
            float V[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
#pragma unroll 1
            for (int sweep = 0; sweep < CLOUD_JACOBI_SWEEPS; sweep++) {
                jacobi_rotate(A, V, 0, 1, 2);
                jacobi_rotate(A, V, 0, 2, 1);
                jacobi_rotate(A, V, 1, 2, 0);
            }
            lam[0] = A[0][0]; lam[1] = A[1][1]; lam[2] = A[2][2];
            order_pair(lam, V, 0, 1);
            order_pair(lam, V, 1, 2);
            order_pair(lam, V, 0, 1);

            const float ln = sqrtf((V[0][0] * V[0][0] + V[1][0] * V[1][0]) + V[2][0] * V[2][0]);
            n[0] = V[0][0] / ln; n[1] = V[1][0] / ln; n[2] = V[2][0] / ln;
            bool flip;
            if (a.oriented) {
                flip = (n[0] * (px - a.ox) + n[1] * (py - a.oy)) + n[2] * (pz - a.oz) < 0.f;
            } else {
                const float lead = n[0] != 0.f ? n[0] : n[1] != 0.f ? n[1] : n[2];
                flip = lead < 0.f;
            }
            if (flip) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }

            if (a.rotations) {
                const float la = sqrtf((V[0][2] * V[0][2] + V[1][2] * V[1][2]) + V[2][2] * V[2][2]);
                const float e[3] = {V[0][2] / la, V[1][2] / la, V[2][2] / la};
                const float b[3] = {n[1] * e[2] - n[2] * e[1], n[2] * e[0] - n[0] * e[2], n[0] * e[1] - n[1] * e[0]};
                // R_i0 = e_i, R_i1 = b_i, R_i2 = n_i
                const float R00 = e[0], R01 = b[0], R02 = n[0], R10 = e[1], R11 = b[1], R12 = n[1], R20 = e[2], R21 = b[2], R22 = n[2];
                const float tr = (R00 + R11) + R22;
                float r, x, y, z;
                if (tr > 0.f) {
                    const float w = sqrtf(tr + 1.f) * 2.f;
                    r = w / 4.f; x = (R21 - R12) / w; y = (R02 - R20) / w; z = (R10 - R01) / w;
                } else if (R00 > R11 && R00 > R22) {
                    const float w = sqrtf(((1.f + R00) - R11) - R22) * 2.f;
                    r = (R21 - R12) / w; x = w / 4.f; y = (R01 + R10) / w; z = (R02 + R20) / w;
                } else if (R11 > R22) {
                    const float w = sqrtf(((1.f + R11) - R00) - R22) * 2.f;
                    r = (R02 - R20) / w; x = (R01 + R10) / w; y = w / 4.f; z = (R12 + R21) / w;
                } else {
                    const float w = sqrtf(((1.f + R22) - R00) - R11) * 2.f;
                    r = (R10 - R01) / w; x = (R02 + R20) / w; y = (R12 + R21) / w; z = w / 4.f;
                }
                const float lq = sqrtf(((r * r + x * x) + y * y) + z * z);
                r = r / lq; x = x / lq; y = y / lq; z = z / lq;
                if (r < 0.f) { r = -r; x = -x; y = -y; z = -z; }
                quat[0] = r; quat[1] = x; quat[2] = y; quat[3] = z;
            }
        }
    }
    if (a.cov6) {
#pragma unroll
        for (int k = 0; k < 6; k++) a.cov6[6 * i + k] = C[k];
    }
    if (a.eigenvalues) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.eigenvalues[3 * i + k] = lam[k];
    }
    if (a.normals) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.normals[3 * i + k] = n[k];
    }
    if (a.rotations) {
#pragma unroll
        for (int k = 0; k < 4; k++) a.rotations[4 * i + k] = quat[k];
    }
}

}  // namespace

int launch_knn(const Launch& L, int P, const float* points, int K, int32_t* idx, float* d2, const KnnScratch& s)
{
    const int nparts = cloud_parts(P);
    const uint32_t nblk = (uint32_t)div_up(P, CLOUD_THREADS), nruns = (uint32_t)cloud_runs(P), ncoarse = (uint32_t)cloud_coarse(P);
    hipLaunchKernelGGL(k_cloud_bounds_part, dim3(nparts), dim3(CLOUD_THREADS), 0, L.stream, P, points, s.parts);
    hipLaunchKernelGGL(k_cloud_bounds, dim3(1), dim3(CLOUD_THREADS), 0, L.stream, nparts, (const float*)s.parts, s.box);
    hipLaunchKernelGGL(k_cloud_keys, dim3(nblk), dim3(CLOUD_THREADS), 0, L.stream, P, points, (const float*)s.box, s.key[0]);
    if (int rc = check_launch(L, "cloud_keys")) return rc;
    SortJob job{{s.key[0], s.key[1]}, {s.val[0], s.val[1]}, s.hist, s.totals, align_up((size_t)P * 4, 256), nullptr, 0, P, 1};
    int res = 0;
    if (int rc = launch_radix_sort_pairs(L, job, /*iota_vals=*/true, CLOUD_KEY_BITS, &res)) return rc;
    hipLaunchKernelGGL(k_cloud_gather, dim3(nblk), dim3(CLOUD_THREADS), 0, L.stream, P, points, (const uint32_t*)s.val[res], s.sorted, s.fine);
    hipLaunchKernelGGL(k_cloud_coarse, dim3((uint32_t)div_up(ncoarse, CLOUD_THREADS / 64)), dim3(CLOUD_THREADS), 0, L.stream, (int)nruns,
                       (int)ncoarse, (const float*)s.fine, s.coarse);
#define GSR_KNN_SEARCH(KMAX)                                                                                                    \
    hipLaunchKernelGGL(k_knn_search<KMAX>, dim3(nruns), dim3(64), 0, L.stream, P, K, (const float4*)s.sorted, (const float*)s.box, \
                       (const float*)s.fine, (const float*)s.coarse, idx, d2)
    if (K <= 4) GSR_KNN_SEARCH(4);
    else if (K <= 8) GSR_KNN_SEARCH(8);
    else if (K <= 16) GSR_KNN_SEARCH(16);
    else GSR_KNN_SEARCH(32);
#undef GSR_KNN_SEARCH
    return check_launch(L, "knn");
}

int launch_cloud_geometry(const Launch& L, const CloudGeometryArgs& a)
{
    hipLaunchKernelGGL(k_cloud_geometry, dim3((uint32_t)div_up(a.P, CLOUD_THREADS)), dim3(CLOUD_THREADS), 0, L.stream, a);
    return check_launch(L, "cloud_geometry");
}

}  // namespace gsr

// ---- the entries: every refusal precedes the first device call, in the header's order ----
using namespace gsr;
#define GSR_ENTRY __attribute__((visibility("default")))   // the unit is built hidden like the kernels' units: only its entries show

GSR_ENTRY size_t gsr_knn_scratch_bytes(int P, int K) { return cloud_sizes_ok(P, K) ? knn_scratch_bytes(P, K) : 0; }

GSR_ENTRY int gsr_knn(int P, const float* points, int K, int32_t* idx, float* d2, void* scratch, size_t scratch_bytes, gsr_stream_t stream)
{
    const char* who = "knn";
    if (!cloud_sizes_ok(P, K))
        return fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes P=%d (at least 1, below 2^30), K=%d (1..%d)", who, P, K, CLOUD_MAX_K);
    if (!points || !idx || !scratch) return fail(GSR_ERR_INVALID, "[gsr] %s: points, idx or scratch is NULL", who);
    // the arrays are carved on 256-B boundaries from the aligned base: an unaligned scratch loses its first bytes
    void* const base = align256(scratch);
    const size_t lost = (size_t)((char*)base - (char*)scratch), need = knn_scratch_bytes(P, K);
    if (scratch_bytes < need + lost)
        return fail(GSR_ERR_CAPACITY, "[gsr] %s: scratch too small (%zu < %zu: gsr_knn_scratch_bytes(%d, %d)%s)", who, scratch_bytes,
                    need + lost, P, K, lost ? " plus the bytes up to the next 256-B boundary" : "");
    const Launch L{(hipStream_t)stream, 0};
    ProfScope ps("knn", L.stream);
    return launch_knn(L, P, points, K, idx, d2, knn_scratch(base, P));
}

GSR_ENTRY int gsr_cloud_geometry(int P, const float* points, int K, const int32_t* knn_idx, int k_s, int k_n, const float* orient_to, float* spacing,
                       float* cov6, float* eigenvalues, float* normals, float* rotations, gsr_stream_t stream)
{
    const char* who = "cloud_geometry";
    if (!cloud_sizes_ok(P, K) || k_s < 1 || k_s > K || k_n < 1 || k_n > K)
        return fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes P=%d (at least 1, below 2^30), K=%d (1..%d), k_s=%d and k_n=%d (1..K)", who, P, K,
                    CLOUD_MAX_K, k_s, k_n);
    if (!points || !knn_idx) return fail(GSR_ERR_INVALID, "[gsr] %s: points or knn_idx is NULL", who);
    if (!spacing && !cov6 && !eigenvalues && !normals && !rotations)
        return fail(GSR_ERR_INVALID, "[gsr] %s: no output: spacing, cov6, eigenvalues, normals and rotations are all NULL", who);
    CloudGeometryArgs a{P, K, k_s, k_n, points, knn_idx, orient_to != nullptr, 0.f, 0.f, 0.f, spacing, cov6, eigenvalues, normals, rotations};
    if (orient_to) {
        a.ox = orient_to[0];
        a.oy = orient_to[1];
        a.oz = orient_to[2];
    }
    const Launch L{(hipStream_t)stream, 0};
    ProfScope ps("cloud_geometry", L.stream);
    return launch_cloud_geometry(L, a);
}
