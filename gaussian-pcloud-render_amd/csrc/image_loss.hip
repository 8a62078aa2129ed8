// image_loss.hip -- the photometric loss of Gaussian-splat training, (1 - lambda) L1 + lambda (1 - SSIM) with the 11 x 11 Gaussian
// window (sigma 1.5, zero padding of 5), per view, and its gradient with respect to the rendered frames (DESIGN.md section 4h;
// include/gsr.h gsr_image_loss_forward / gsr_image_loss_backward has the definition).  With ss = 2 the frames are twice the loss's
// resolution each way: the loader averages every 2 x 2 block (what the caller's bilinear down-filter does at rate 2) and the
// backward's store hands every source pixel a quarter.
//
// Mapping: one workgroup of 256 threads per (IL_TILE_W x IL_TILE_H tile, channel, view).
//   load     the tile plus a halo of 5 (REG_W x REG_H = 42 x 42), zero outside the image, into LDS: aligned groups of four pixels,
//            16-B loads where the rows are 16-B aligned (W % 4 == 0 and aligned pointers), element loads elsewhere
//   rows     an item is four neighbouring outputs of one region row (42 x 8 items): 14 values per input from LDS, the products
//            x x, y y, x y once per value, 11 fused multiply-adds per output and quantity -- (x, y) and (x x, y y) as pairs on the
//            packed instruction -- and one 16-B LDS store per quantity
//   columns  a thread owns four neighbouring pixels of one tile row: 11 16-B LDS reads per quantity, packed multiply-adds again
//   pixel    forward: the SSIM map m, its three derivative maps A B C (stored into the state, 16-B stores where aligned) and the three
//            sums; backward: the gradient from conv(A), conv(B), conv(C), x and y
// LDS rows: the inputs' row stride is SX = 43 words -- a 32-lane group of the row pass is 4 rows x 8 items at word offsets
// 43 row + 4 item + j, and 43 = 11 (mod 32) puts the four rows on the four residues mod 4: 32 banks, no conflict (a stride of 42 or 44
// runs pairs of rows into the same banks).  The row sums' stride is HS = 32 words: the row pass stores and the column pass reads them
// 16 B per lane, eight lanes to a row, and the four rows a 16-lane read group spans (r, r + 1, r + 2, r + 3 at word offsets
// 0, 48, 80, 96 mod 64) cover the 64 banks once.
//
// Sums: a thread adds its four pixels in float64, the wave reduces with shuffles, thread 0 adds the four waves in order and stores the
// three float64 partials of the workgroup; k_image_loss_sum (one workgroup per view) adds a view's partials by index -- thread t those
// with index = t mod 256, in increasing order, then a fixed tree -- and rounds to float32 once.  No atomics: the bits do not depend
// on the launch order, on V, or on the other views.  The metrics-only forward (no state block to hold partials) is one workgroup per
// view that walks the view's (tile, channel) pairs with the same tile code and adds every partial to the accumulator k_image_loss_sum's
// thread would have used, in the same order: the same bits, at the speed of one compute unit per view.
#include "common.hpp"
#include "image_loss.hpp"

namespace gsr {

constexpr int REG_W = IL_TILE_W + 2 * IL_HALO;
constexpr int REG_H = IL_TILE_H + 2 * IL_HALO;
constexpr int SX = REG_W + 1;               // 43: see above
constexpr int HS = IL_TILE_W;               // 32
constexpr int ROW_GROUPS = IL_TILE_W / 4;   // row-pass items per region row, threads per tile row
constexpr int LOAD_GROUPS = 12;             // aligned groups of four covering the region's columns [tx0 - 8, tx0 + 40)
static_assert(IL_TILE_W == 32 && IL_TILE_H * ROW_GROUPS == IL_THREADS, "one thread per four pixels of the tile");
static_assert(IL_HALO == 5 && LOAD_GROUPS * 4 >= REG_W + 3, "the aligned load groups cover the region");

// g[k] = exp(-(k - 5)^2 / 4.5) / sum, rounded from float64
__device__ constexpr float IL_G[11] = {1.0283800845e-03f, 7.5987581352e-03f, 3.6000772128e-02f, 1.0936068951e-01f, 2.1300553771e-01f,
                                       2.6601172486e-01f, 2.1300553771e-01f, 1.0936068951e-01f, 3.6000772128e-02f, 7.5987581352e-03f,
                                       1.0283800845e-03f};
constexpr float IL_C1 = 1e-4f, IL_C2 = 9e-4f;

typedef float il_f4 __attribute__((ext_vector_type(4)));
typedef float il_f2 __attribute__((ext_vector_type(2)));

// two fused multiply-adds in one instruction (v_pk_fma_f32): each half is rounded like fmaf
__device__ __forceinline__ il_f2 il_fma2(float g, il_f2 v, il_f2 acc) { return __builtin_elementwise_fma(il_f2{g, g}, v, acc); }

// Four loss-resolution pixels gx .. gx + 3 of row gy (0 <= gy < H; gx % 4 == 0, anywhere) of a plane: [H][W] (SS 1) or the
// [2 H][2 W] frame whose 2 x 2 blocks are averaged (SS 2).  Pixels outside [0, W) are 0.  VEC: rows are 16-B aligned and W % 4 == 0,
// so a group lies inside the row or outside it.
template <int SS, bool VEC>
__device__ __forceinline__ void il_load4(const float* __restrict__ plane, int W, int gx, int gy, float v[4])
{
    if constexpr (SS == 1) {
        const float* row = plane + (size_t)gy * (size_t)W;
        if (VEC && gx >= 0 && gx < W) {
            const il_f4 q = *reinterpret_cast<const il_f4*>(row + gx);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = (gx + j >= 0 && gx + j < W) ? row[gx + j] : 0.f;
        }
    } else {
        const float* r0 = plane + (size_t)(2 * gy) * (size_t)(2 * W);
        const float* r1 = r0 + 2 * W;
        if (VEC && gx >= 0 && gx < W) {
            const il_f4 a0 = *reinterpret_cast<const il_f4*>(r0 + 2 * gx), a1 = *reinterpret_cast<const il_f4*>(r0 + 2 * gx + 4);
            const il_f4 b0 = *reinterpret_cast<const il_f4*>(r1 + 2 * gx), b1 = *reinterpret_cast<const il_f4*>(r1 + 2 * gx + 4);
            v[0] = ((a0.x + a0.y) + (b0.x + b0.y)) * 0.25f;
            v[1] = ((a0.z + a0.w) + (b0.z + b0.w)) * 0.25f;
            v[2] = ((a1.x + a1.y) + (b1.x + b1.y)) * 0.25f;
            v[3] = ((a1.z + a1.w) + (b1.z + b1.w)) * 0.25f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int c = 2 * (gx + j);
                v[j] = (gx + j >= 0 && gx + j < W) ? ((r0[c] + r0[c + 1]) + (r1[c] + r1[c + 1])) * 0.25f : 0.f;
            }
        }
    }
}

// the region of one plane into LDS (row stride SX), zero outside the image
template <int SS, bool VEC>
__device__ __forceinline__ void il_fill(float* __restrict__ s, const float* __restrict__ plane, int W, int H, int tx0, int ty0)
{
    for (int item = threadIdx.x; item < REG_H * LOAD_GROUPS; item += IL_THREADS) {
        const int ly = item / LOAD_GROUPS, grp = item % LOAD_GROUPS;
        const int gy = ty0 + ly - IL_HALO, gx = tx0 - 8 + grp * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (gy >= 0 && gy < H) il_load4<SS, VEC>(plane, W, gx, gy, v);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int lx = grp * 4 + j - 3;   // gx + j - (tx0 - IL_HALO)
            if (lx >= 0 && lx < REG_W) s[ly * SX + lx] = v[j];
        }
    }
}

// 11-tap sums down the columns of the row sums of quantity q, for the thread's four pixels
__device__ __forceinline__ il_f4 il_columns(const float* __restrict__ h, int q, int r, int cg)
{
    il_f2 lo = {0.f, 0.f}, hi = {0.f, 0.f};
    const float* p = h + (q * REG_H + r) * HS + cg * 4;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const il_f4 t = *reinterpret_cast<const il_f4*>(p + k * HS);
        lo = il_fma2(IL_G[k], t.xy, lo);
        hi = il_fma2(IL_G[k], t.zw, hi);
    }
    return il_f4{lo.x, lo.y, hi.x, hi.y};
}

struct IlTile {
    int view, ch, tx0, ty0;
};
__device__ __forceinline__ IlTile il_tile(int part, int view, int W)
{
    const int tiles_x = (W + IL_TILE_W - 1) / IL_TILE_W, tile = part / 3;
    return IlTile{view, part % 3, (tile % tiles_x) * IL_TILE_W, (tile / tiles_x) * IL_TILE_H};
}

// LDS of the forward: the two inputs' regions, the five row sums, the waves' sums
struct IlFwdLds {
    float sx[REG_H * SX], sy[REG_H * SX];
    __attribute__((aligned(16))) float h[5 * REG_H * HS];
    double red[IL_THREADS / 64][IL_SUMS];
};

// One (tile, channel) of the forward.  maps != NULL: view 0's maps, A B C of the tile's pixels are stored.  Returns the three sums
// over the tile's pixels in thread 0 (sums[]).
template <int SS, bool VEC>
__device__ __forceinline__ void il_forward_tile(IlFwdLds& S, const ImageLossArgs& a, const IlTile t, float* __restrict__ maps,
                                                double sums[IL_SUMS])
{
    const size_t HW = (size_t)a.W * (size_t)a.H;
    const size_t plane = (size_t)t.view * 3 + (size_t)t.ch;
    __syncthreads();   // (the metrics-only walk: the previous tile's readers are done)
    il_fill<SS, VEC>(S.sx, a.image + plane * HW * (size_t)(SS * SS), a.W, a.H, t.tx0, t.ty0);
    il_fill<1, VEC>(S.sy, a.target + plane * HW, a.W, a.H, t.tx0, t.ty0);
    __syncthreads();
    // rows: mu1 mu2 E[xx] E[yy] E[xy] along x
    for (int item = threadIdx.x; item < REG_H * ROW_GROUPS; item += IL_THREADS) {
        const int row = item / ROW_GROUPS, cg = item % ROW_GROUPS;
        const float* px = S.sx + row * SX + cg * 4;
        const float* py = S.sy + row * SX + cg * 4;
        il_f2 v[14], vv[14];   // (x, y), (x x, y y): the pairs go through the packed multiply-add
        float xy[14];
#pragma unroll
        for (int i = 0; i < 14; i++) {
            v[i] = il_f2{px[i], py[i]};
            vv[i] = v[i] * v[i];
            xy[i] = v[i].x * v[i].y;
        }
        float acc[5][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            il_f2 s01 = {0.f, 0.f}, s23 = {0.f, 0.f};
            float s4 = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                s01 = il_fma2(IL_G[k], v[j + k], s01);
                s23 = il_fma2(IL_G[k], vv[j + k], s23);
                s4 = fmaf(IL_G[k], xy[j + k], s4);
            }
            acc[0][j] = s01.x; acc[1][j] = s01.y; acc[2][j] = s23.x; acc[3][j] = s23.y; acc[4][j] = s4;
        }
#pragma unroll
        for (int q = 0; q < 5; q++)
            *reinterpret_cast<il_f4*>(S.h + (q * REG_H + row) * HS + cg * 4) = il_f4{acc[q][0], acc[q][1], acc[q][2], acc[q][3]};
    }
    __syncthreads();
    // columns and the pixels
    const int cg = threadIdx.x % ROW_GROUPS, r = threadIdx.x / ROW_GROUPS;
    const il_f4 mu1v = il_columns(S.h, 0, r, cg), mu2v = il_columns(S.h, 1, r, cg), exxv = il_columns(S.h, 2, r, cg),
                eyyv = il_columns(S.h, 3, r, cg), exyv = il_columns(S.h, 4, r, cg);
    const int gy = t.ty0 + r, gx0 = t.tx0 + cg * 4;
    float A[4], B[4], C[4];
    double d_l1 = 0.0, d_m = 0.0, d_se = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float mu1 = mu1v[j], mu2 = mu2v[j];
        const float x = S.sx[(r + IL_HALO) * SX + cg * 4 + IL_HALO + j], y = S.sy[(r + IL_HALO) * SX + cg * 4 + IL_HALO + j];
        // (written so that x == y gives n1 == d1 and n2 == d2 bit for bit: m = 1, A = 0, and the backward's SSIM term is exactly 0)
        const float s1 = fmaf(-mu1, mu1, exxv[j]), s2 = fmaf(-mu2, mu2, eyyv[j]), s12 = fmaf(-mu1, mu2, exyv[j]);
        const float n1 = 2.f * mu1 * mu2 + IL_C1, d1 = (mu1 * mu1 + mu2 * mu2) + IL_C1;
        const float n2 = 2.f * s12 + IL_C2, d2 = (s1 + s2) + IL_C2;
        // (the two ratios are true divisions -- exactly 1 for equal operands; the reciprocals are the hardware's, 1 ulp)
        const float r1 = n1 / d1, r2 = n2 / d2, id1 = __builtin_amdgcn_rcpf(d1), id2 = __builtin_amdgcn_rcpf(d2);
        const float m = r1 * r2;
        const float dmu1 = 2.f * id1 * (mu2 * r2 - mu1 * m);   // dm/dmu1 at fixed s1, s12
        B[j] = -(m * id2);                                     // dm/ds1
        C[j] = 2.f * r1 * id2;                                 // dm/ds12
        A[j] = (dmu1 - 2.f * mu1 * B[j]) - mu2 * C[j];
        if (gy < a.H && gx0 + j < a.W) {
            const float d = x - y;
            d_l1 += (double)fabsf(d);
            d_m += (double)m;
            d_se += (double)d * (double)d;
        }
    }
    if (maps != nullptr && gy < a.H) {
        float* mp = maps + (size_t)t.view * 9 * HW + (size_t)t.ch * HW + (size_t)gy * (size_t)a.W + gx0;
        if (VEC && gx0 < a.W) {
            *reinterpret_cast<il_f4*>(mp) = il_f4{A[0], A[1], A[2], A[3]};
            *reinterpret_cast<il_f4*>(mp + 3 * HW) = il_f4{B[0], B[1], B[2], B[3]};
            *reinterpret_cast<il_f4*>(mp + 6 * HW) = il_f4{C[0], C[1], C[2], C[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (gx0 + j < a.W) {
                    mp[j] = A[j];
                    mp[3 * HW + j] = B[j];
                    mp[6 * HW + j] = C[j];
                }
        }
    }
    // the workgroup's three sums: shuffles inside the wave, the four waves in order
#pragma unroll
    for (int d = 1; d <= 32; d <<= 1) {
        d_l1 += __shfl_xor(d_l1, d, 64);
        d_m += __shfl_xor(d_m, d, 64);
        d_se += __shfl_xor(d_se, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        S.red[threadIdx.x >> 6][0] = d_l1;
        S.red[threadIdx.x >> 6][1] = d_m;
        S.red[threadIdx.x >> 6][2] = d_se;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < IL_SUMS; q++) sums[q] = ((S.red[0][q] + S.red[1][q]) + S.red[2][q]) + S.red[3][q];
    }
}

// acc[q][t]: the sum of the partials with index = t (mod IL_THREADS), in increasing order.  Adds them in a fixed tree and writes the
// view's four terms.
__device__ __forceinline__ void il_finish(double (*acc)[IL_THREADS], double n, float lambda, float* __restrict__ out4)
{
    for (int s = IL_THREADS / 2; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int q = 0; q < IL_SUMS; q++) acc[q][threadIdx.x] += acc[q][threadIdx.x + s];
    }
    if (threadIdx.x == 0) {
        const float l1 = (float)(acc[0][0] / n), ssim = (float)(acc[1][0] / n), mse = (float)(acc[2][0] / n);
        out4[0] = l1;
        out4[1] = ssim;
        out4[2] = mse;
        out4[3] = (float)((1.0 - (double)lambda) * (double)l1 + (double)lambda * (1.0 - (double)ssim));
    }
}

// (three waves per SIMD, i.e. the three workgroups per compute unit the LDS allows: 168 registers and six spilled ones instead of 185 --
// measured 0.98 against 1.09 ms for 12 views at 1080p, profiles/r23_image_loss.txt)
template <int SS, bool VEC>
__global__ __launch_bounds__(IL_THREADS, 3) void k_image_loss_forward(ImageLossArgs a, float* maps, double* partials, int nparts)
{
    __shared__ IlFwdLds S;
    double sums[IL_SUMS];
    il_forward_tile<SS, VEC>(S, a, il_tile((int)blockIdx.x, (int)blockIdx.y, a.W), maps, sums);
    if (threadIdx.x == 0) {
        double* p = partials + ((size_t)blockIdx.y * (size_t)nparts + blockIdx.x) * IL_SUMS;
#pragma unroll
        for (int q = 0; q < IL_SUMS; q++) p[q] = sums[q];
    }
}

__global__ __launch_bounds__(IL_THREADS) void k_image_loss_sum(const double* __restrict__ partials, int nparts, double n, float lambda,
                                                               float* __restrict__ loss_terms)
{
    __shared__ double acc[IL_SUMS][IL_THREADS];
    const double* p = partials + (size_t)blockIdx.x * (size_t)nparts * IL_SUMS;
    double s[IL_SUMS] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nparts; i += IL_THREADS)
#pragma unroll
        for (int q = 0; q < IL_SUMS; q++) s[q] += p[(size_t)i * IL_SUMS + q];
#pragma unroll
    for (int q = 0; q < IL_SUMS; q++) acc[q][threadIdx.x] = s[q];
    il_finish(acc, n, lambda, loss_terms + (size_t)blockIdx.x * 4);
}

// the metrics-only forward: one workgroup per view
template <int SS, bool VEC>
__global__ __launch_bounds__(IL_THREADS) void k_image_loss_metrics(ImageLossArgs a, int nparts, double n, float lambda,
                                                                   float* __restrict__ loss_terms)
{
    __shared__ IlFwdLds S;
    __shared__ double acc[IL_SUMS][IL_THREADS];
#pragma unroll
    for (int q = 0; q < IL_SUMS; q++) acc[q][threadIdx.x] = 0.0;
    for (int part = 0; part < nparts; part++) {
        double sums[IL_SUMS];
        il_forward_tile<SS, VEC>(S, a, il_tile(part, (int)blockIdx.x, a.W), nullptr, sums);
        if (threadIdx.x == 0)   // (the only thread that touches acc before il_finish's first barrier)
#pragma unroll
            for (int q = 0; q < IL_SUMS; q++) acc[q][part % IL_THREADS] += sums[q];
    }
    il_finish(acc, n, lambda, loss_terms + (size_t)blockIdx.x * 4);
}

struct IlBwdLds {
    float sm[3][REG_H * SX];
    __attribute__((aligned(16))) float h[3 * REG_H * HS];
};

// cl1 = (1 - lambda) / (3 H W), cs = -lambda / (3 H W)
template <int SS, bool VEC>
__global__ __launch_bounds__(IL_THREADS) void k_image_loss_backward(ImageLossArgs a, const float* __restrict__ maps,
                                                                    const float* __restrict__ dL_dloss, float cl1, float cs,
                                                                    float* __restrict__ dL_dimage)
{
    __shared__ IlBwdLds S;
    const IlTile t = il_tile((int)blockIdx.x, (int)blockIdx.y, a.W);
    const size_t HW = (size_t)a.W * (size_t)a.H;
    const size_t plane = (size_t)t.view * 3 + (size_t)t.ch;
#pragma unroll
    for (int m = 0; m < 3; m++)
        il_fill<1, VEC>(S.sm[m], maps + (size_t)t.view * 9 * HW + ((size_t)m * 3 + (size_t)t.ch) * HW, a.W, a.H, t.tx0, t.ty0);
    __syncthreads();
    for (int item = threadIdx.x; item < REG_H * ROW_GROUPS; item += IL_THREADS) {
        const int row = item / ROW_GROUPS, cg = item % ROW_GROUPS;
        const int at = row * SX + cg * 4;
        il_f2 ab[14];   // (A, B): the pair goes through the packed multiply-add
        float c[14];
#pragma unroll
        for (int i = 0; i < 14; i++) {
            ab[i] = il_f2{S.sm[0][at + i], S.sm[1][at + i]};
            c[i] = S.sm[2][at + i];
        }
        float acc[3][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            il_f2 s01 = {0.f, 0.f};
            float s2 = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                s01 = il_fma2(IL_G[k], ab[j + k], s01);
                s2 = fmaf(IL_G[k], c[j + k], s2);
            }
            acc[0][j] = s01.x; acc[1][j] = s01.y; acc[2][j] = s2;
        }
#pragma unroll
        for (int m = 0; m < 3; m++)
            *reinterpret_cast<il_f4*>(S.h + (m * REG_H + row) * HS + cg * 4) = il_f4{acc[m][0], acc[m][1], acc[m][2], acc[m][3]};
    }
    __syncthreads();
    const int cg = threadIdx.x % ROW_GROUPS, r = threadIdx.x / ROW_GROUPS;
    const int gy = t.ty0 + r, gx0 = t.tx0 + cg * 4;
    if (gy >= a.H || gx0 >= a.W) return;
    const il_f4 cA = il_columns(S.h, 0, r, cg), cB = il_columns(S.h, 1, r, cg), cC = il_columns(S.h, 2, r, cg);
    float x[4], y[4], g[4];
    il_load4<SS, VEC>(a.image + plane * HW * (size_t)(SS * SS), a.W, gx0, gy, x);
    il_load4<1, VEC>(a.target + plane * HW, a.W, gx0, gy, y);
    const float scale = dL_dloss != nullptr ? dL_dloss[t.view] : 1.f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float d = x[j] - y[j];
        const float sgn = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
        // (separate products, not fused: with x == y the two cancel exactly)
        const float base = cl1 * sgn + cs * (cA[j] + (2.f * x[j] * cB[j] + y[j] * cC[j]));
        g[j] = base * scale;
        if (SS == 2) g[j] *= 0.25f;
    }
    if constexpr (SS == 1) {
        float* o = dL_dimage + plane * HW + (size_t)gy * (size_t)a.W + gx0;
        if (VEC) {
            *reinterpret_cast<il_f4*>(o) = il_f4{g[0], g[1], g[2], g[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (gx0 + j < a.W) o[j] = g[j];
        }
    } else {
        float* o0 = dL_dimage + plane * HW * 4 + (size_t)(2 * gy) * (size_t)(2 * a.W) + 2 * gx0;
        float* o1 = o0 + 2 * a.W;
        if (VEC) {
            const il_f4 lo = {g[0], g[0], g[1], g[1]}, hi = {g[2], g[2], g[3], g[3]};
            *reinterpret_cast<il_f4*>(o0) = lo;
            *reinterpret_cast<il_f4*>(o0 + 4) = hi;
            *reinterpret_cast<il_f4*>(o1) = lo;
            *reinterpret_cast<il_f4*>(o1 + 4) = hi;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (gx0 + j < a.W) {
                    o0[2 * j] = g[j];
                    o0[2 * j + 1] = g[j];
                    o1[2 * j] = g[j];
                    o1[2 * j + 1] = g[j];
                }
        }
    }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int launch_image_loss_forward(const Launch& L, const ImageLossArgs& a, float lambda, float* loss_terms, double* partials, float* maps)
{
    const int nparts = (int)il_parts(a.W, a.H);
    const double n = 3.0 * (double)a.W * (double)a.H;
    const bool vec = a.W % 4 == 0 && aligned16(a.image) && aligned16(a.target) && aligned16(maps);
    const int variant = (a.ss == 2 ? 2 : 0) + (vec ? 1 : 0);
    if (partials != nullptr) {
        const dim3 grid((unsigned)nparts, (unsigned)a.V);
        switch (variant) {
        case 0: hipLaunchKernelGGL((k_image_loss_forward<1, false>), grid, dim3(IL_THREADS), 0, L.stream, a, maps, partials, nparts); break;
        case 1: hipLaunchKernelGGL((k_image_loss_forward<1, true>), grid, dim3(IL_THREADS), 0, L.stream, a, maps, partials, nparts); break;
        case 2: hipLaunchKernelGGL((k_image_loss_forward<2, false>), grid, dim3(IL_THREADS), 0, L.stream, a, maps, partials, nparts); break;
        default: hipLaunchKernelGGL((k_image_loss_forward<2, true>), grid, dim3(IL_THREADS), 0, L.stream, a, maps, partials, nparts); break;
        }
        if (int e = check_launch(L, "image_loss_forward")) return e;
        hipLaunchKernelGGL(k_image_loss_sum, dim3((unsigned)a.V), dim3(IL_THREADS), 0, L.stream, partials, nparts, n, lambda, loss_terms);
        return check_launch(L, "image_loss_sum");
    }
    const dim3 grid((unsigned)a.V);
    switch (variant) {
    case 0: hipLaunchKernelGGL((k_image_loss_metrics<1, false>), grid, dim3(IL_THREADS), 0, L.stream, a, nparts, n, lambda, loss_terms); break;
    case 1: hipLaunchKernelGGL((k_image_loss_metrics<1, true>), grid, dim3(IL_THREADS), 0, L.stream, a, nparts, n, lambda, loss_terms); break;
    case 2: hipLaunchKernelGGL((k_image_loss_metrics<2, false>), grid, dim3(IL_THREADS), 0, L.stream, a, nparts, n, lambda, loss_terms); break;
    default: hipLaunchKernelGGL((k_image_loss_metrics<2, true>), grid, dim3(IL_THREADS), 0, L.stream, a, nparts, n, lambda, loss_terms); break;
    }
    return check_launch(L, "image_loss_metrics");
}

int launch_image_loss_backward(const Launch& L, const ImageLossArgs& a, float lambda, const float* dL_dloss, const float* maps,
                               float* dL_dimage)
{
    const int nparts = (int)il_parts(a.W, a.H);
    const double n = 3.0 * (double)a.W * (double)a.H;
    const float cl1 = (float)((1.0 - (double)lambda) / n), cs = (float)(-(double)lambda / n);
    const bool vec = a.W % 4 == 0 && aligned16(a.image) && aligned16(a.target) && aligned16(maps) && aligned16(dL_dimage);
    const dim3 grid((unsigned)nparts, (unsigned)a.V);
    switch ((a.ss == 2 ? 2 : 0) + (vec ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((k_image_loss_backward<1, false>), grid, dim3(IL_THREADS), 0, L.stream, a, maps, dL_dloss, cl1, cs, dL_dimage); break;
    case 1: hipLaunchKernelGGL((k_image_loss_backward<1, true>), grid, dim3(IL_THREADS), 0, L.stream, a, maps, dL_dloss, cl1, cs, dL_dimage); break;
    case 2: hipLaunchKernelGGL((k_image_loss_backward<2, false>), grid, dim3(IL_THREADS), 0, L.stream, a, maps, dL_dloss, cl1, cs, dL_dimage); break;
    default: hipLaunchKernelGGL((k_image_loss_backward<2, true>), grid, dim3(IL_THREADS), 0, L.stream, a, maps, dL_dloss, cl1, cs, dL_dimage); break;
    }
    return check_launch(L, "image_loss_backward");
}

}  // namespace gsr
