// det_backward.hip -- the steps of the deterministic colour backward around the storing render backward
// (gsr_backward_batch_det).
//
// The atomic backward (render_bwd.hip) adds every (quadrant, entry) partial sum into the Gaussian's 64-B record with float atomics,
// in whatever order the waves of the launch arrive: the reference does the same per pixel (CR/backward.cu:523-554), and neither is
// repeatable to the last bit.  The partial sums themselves do not depend on the schedule, so the ordered path keeps the kernel and
// changes only where they land:
//   k_det_prefix   slot_base[t] = consumed list entries of the tiles before t (exclusive prefix sum of tile_need, one workgroup per
//                  view): consumed position i = slot_base[tile] + position in the tile's list
//   k_det_emit     for every consumed position: key = Gaussian id (point_list), value = i (implicit), and flags[i] = 0
//   radix sort     the library's own stable u32 / u32 sort (sort.hip) by Gaussian id, ceil(log2 P) key bits: a Gaussian's consumed
//                  positions become one run, ascending, i.e. by tile and then by depth inside the tile
//   k_render_backward<MODE, 0, RenderBwdDet>   stores the nine sums of (position, quadrant) into slot i * 4 + quadrant, marks byte
//                  `quadrant` of flags[i]
//   k_det_reduce   walks each run in order, adds the marked quadrants 0, 1, 2, 3 of every position in a float64 register and writes
//                  the Gaussian's record, rounded to float32 once, with plain stores
// Slots a unit skipped (footprint test, no pixel hit in the entry's group of four, beyond the quadrant's n_contrib) are never
// written; they are told apart by the flag word -- 4 B per position to clear instead of 256 B -- and are not read either.
// Every step is a launch of its own on the caller's stream: no device-wide wait, no float atomic.
// The deterministic channels backward (gsr_backward_batch_channels_det) runs the same steps with k_render_backward<MODE, NX,
// RenderBwdX, RenderBwdDet>, which also stores dL/d extra of every (position, quadrant) into an extra slot, and two more:
//   k_det_reduce_x  the same walk over the same sorted runs on the extra slots, per view, into the caller's per-view rows or the
//                   staging of the rows the views share
//   k_det_viewsum   the staged rows of the views added for v = 0 .. V - 1 in float64, rounded once
#include <algorithm>
#include <vector>

#include "common.hpp"

namespace gsr {

// ---- consumed positions ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_det_prefix(int T, const uint32_t* __restrict__ need, size_t iv_stride,
                                                      uint32_t* __restrict__ slot_base, uint64_t* __restrict__ count, size_t d_stride,
                                                      uint32_t cap)
{
    need = at_view(need, iv_stride, blockIdx.x);
    slot_base = at_view(slot_base, d_stride, blockIdx.x);
    count = at_view(count, d_stride, blockIdx.x);
    __shared__ uint32_t wsum[16];
    const int per = (T + 1023) / 1024;
    const int t0 = (int)threadIdx.x * per, t1 = t0 + per < T ? t0 + per : T;
    uint32_t s = 0;
    for (int t = t0; t < t1; t++) s += need[t];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t n = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += n;
    }
    if (lane == 63u) wsum[w] = inc;
    __syncthreads();
    uint32_t run = inc - s, total = 0;
    for (uint32_t i = 0; i < 16u; i++) {
        if (i < w) run += wsum[i];
        total += wsum[i];
    }
    for (int t = t0; t < t1; t++) {
        slot_base[t] = run;
        run += need[t];
    }
    if (threadIdx.x == 0) {
        slot_base[T] = total;
        count[0] = total < cap ? total : cap;   // (never more than the lists hold, which the block was sized for)
    }
}

// one wave per tile: the ids of its consumed entries become the sort keys, their flag words are cleared
__global__ __launch_bounds__(256) void k_det_emit(int T, const uint2* __restrict__ ranges, size_t iv_stride,
                                                   const uint32_t* __restrict__ point_list, size_t b_stride,
                                                   const uint32_t* __restrict__ slot_base, uint32_t* __restrict__ key,
                                                   uint32_t* __restrict__ flags, size_t d_stride, uint32_t cap)
{
    const uint32_t view = blockIdx.y, lane = threadIdx.x & 63u;
    const int tile = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (tile >= T) return;
    slot_base = at_view(slot_base, d_stride, view);
    key = at_view(key, d_stride, view);
    flags = at_view(flags, d_stride, view);
    const uint32_t lo = slot_base[tile], n = slot_base[tile + 1] - lo;
    if (n == 0) return;
    const uint32_t* plist = at_view(point_list, b_stride, view) + at_view(ranges, iv_stride, view)[tile].x;
    for (uint32_t i = lane; i < n; i += 64u) {
        const size_t c = (size_t)lo + i;
        if (c < (size_t)cap) {
            key[c] = plist[i];
            flags[c] = 0u;
        }
    }
}

int launch_det_prepare(const Launch& L, const Batch& B, const DetView& D, size_t d_stride, const uint32_t* point_list, int T)
{
    hipLaunchKernelGGL(k_det_prefix, dim3(B.V), dim3(1024), 0, L.stream, T, (const uint32_t*)B.iv.tile_need, B.iv_stride, D.slot_base,
                       D.count, d_stride, (uint32_t)D.cap);
    if (int e = check_launch(L, "det_prefix")) return e;
    hipLaunchKernelGGL(k_det_emit, dim3((unsigned)div_up(T, 4), B.V), dim3(256), 0, L.stream, T, (const uint2*)B.iv.ranges, B.iv_stride,
                       point_list, B.b_stride, (const uint32_t*)D.slot_base, D.key[0], D.flags, d_stride, (uint32_t)D.cap);
    return check_launch(L, "det_emit");
}

// key bits of the sort by Gaussian id: ids are < P
static int id_bits(int P)
{
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < (int64_t)P) bits++;
    return bits;
}

int launch_det_sort(const Launch& L, const Batch& B, const DetView& D, size_t d_stride, int P, int* result_buffer)
{
    const SortJob job{{D.key[0], D.key[1]}, {D.val[0], D.val[1]}, D.hist, D.totals, d_stride, D.count, d_stride, D.cap, B.V};
    return launch_radix_sort_pairs(L, job, /*iota_vals=*/true, id_bits(P), result_buffer);
}

// ---- the ordered reduction ---------------------------------------------------------------------------------------------------
// Sixteen lanes per sorted element, lane c = word c of a slot / record (one 64-B line per load).  The sixteen lanes of a run's FIRST
// element walk the whole run; the others leave.  The order of the additions -- positions ascending (tile, then depth), quadrants
// 0..3 inside a position, unmarked slots left out -- is the contract: it depends on nothing but the lists.  The running sum is kept
// in float64 and rounded to float32 once, when the record is written: the order is fixed anyway, and a float32 running sum taken
// tile by tile measured 3 to 13 % MORE error against the float64 backward on the colour sums than the atomic path's arrival order
// (neighbouring tiles' partials of one splat are alike in size and sign); with the float64 sum the only float32 roundings left
// are those inside the partial sums, which both paths share.
constexpr int DET_REDUCE_BLOCKS = 4096;
__global__ __launch_bounds__(256) void k_det_reduce(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                     const uint32_t* __restrict__ flags, const float* __restrict__ part,
                                                     const uint64_t* __restrict__ count, size_t d_stride, float* __restrict__ grad_rec,
                                                     size_t gr_stride)
{
    const uint32_t view = blockIdx.y;
    key = at_view(key, d_stride, view);
    val = at_view(val, d_stride, view);
    flags = at_view(flags, d_stride, view);
    part = at_view(part, d_stride, view);
    grad_rec = at_view(grad_rec, gr_stride, view);
    const uint64_t n = *at_view(count, d_stride, view);
    const uint32_t c = threadIdx.x & 15u, sub = (threadIdx.x >> 4) & 3u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 4); i0 < n; i0 += (uint64_t)gridDim.x * 16u) {
        const uint32_t id = key[i0];
        if (i0 != 0 && key[i0 - 1] == id) continue;   // not the first element of its run
        double acc = 0.0;
        // sixteen elements of the run at a time: lane c fetches element c's position and flag word (one round trip for sixteen),
        // then the slots are read eight positions ahead of the additions, which stay in list order
        for (uint64_t i = i0;; i += 16u) {
            const uint64_t j = i + c;
            const bool in = j < n && key[j] == id;
            uint32_t pos = 0, f = 0;
            if (in) {
                pos = val[j];
                f = flags[pos];
            }
            // (keys are sorted: the lanes inside the run are the first `cnt` of the sixteen)
            const uint32_t cnt = (uint32_t)__popc((uint32_t)(__ballot(in) >> (16u * sub)) & 0xFFFFu);
            for (uint32_t k0 = 0; k0 < cnt; k0 += 8u) {
                float v[8][4];
                uint32_t fk[8];
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
                    const uint32_t pk = (uint32_t)__shfl((int)pos, (int)(k0 + k), 16);
                    fk[k] = k0 + k < cnt ? (uint32_t)__shfl((int)f, (int)(k0 + k), 16) : 0u;
                    const float* s = part + (size_t)pk * (4 * DET_SLOT_WORDS) + c;
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++) v[k][q] = (fk[k] >> (8u * q)) & 0xFFu ? s[q * DET_SLOT_WORDS] : 0.f;
                }
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++)
                        if ((fk[k] >> (8u * q)) & 0xFFu) acc += (double)v[k][q];
                }
            }
            if (cnt < 16u) break;
        }
        grad_rec[(size_t)id * GRAD_REC_WORDS + c] = (float)acc;   // (words 9..15: sums of the slots' zero padding)
    }
}

int launch_det_reduce(const Launch& L, const Batch& B, const DetView& D, size_t d_stride, int sorted_buffer)
{
    int64_t blocks = div_up(D.cap, 16);
    if (blocks > DET_REDUCE_BLOCKS) blocks = DET_REDUCE_BLOCKS;
    hipLaunchKernelGGL(k_det_reduce, dim3((unsigned)blocks, B.V), dim3(256), 0, L.stream, (const uint32_t*)D.key[sorted_buffer],
                       (const uint32_t*)D.val[sorted_buffer], (const uint32_t*)D.flags, (const float*)D.part, (const uint64_t*)D.count,
                       d_stride, B.grad_rec, B.gr_stride);
    return check_launch(L, "det_reduce");
}

// Self-test of k_det_reduce: random runs, random marks, random partial sums; the host adds the same floats in the same order.
int selftest_det_reduce(hipStream_t stream)
{
    const int P = 997, n = 20011;
    std::vector<uint32_t> hk(n), hv(n), hf(n);
    std::vector<float> hp((size_t)n * 4 * DET_SLOT_WORDS), want((size_t)P * GRAD_REC_WORDS, -1.f), got(want.size());
    uint32_t x = 2463534242u;
    const auto rnd = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    // sorted keys with runs of 1..80 elements and gaps between the ids
    int used = 0;
    for (uint32_t id = rnd() % 3u; id < (uint32_t)P && used < n; id += 1u + rnd() % 3u) {
        const int len = 1 + (int)(rnd() % 80u);
        for (int j = 0; j < len && used < n; j++) hk[used++] = id;
    }
    // positions: a strided walk through [0, n) keeps them distinct; ascending inside a run, as the stable sort leaves them
    for (int j = 0; j < used; j++) hv[j] = (uint32_t)(((uint64_t)j * 7919u) % (uint32_t)n);
    for (int a = 0, b = 0; a < used; a = b) {
        for (b = a; b < used && hk[b] == hk[a];) b++;
        std::sort(hv.begin() + a, hv.begin() + b);
    }
    for (int j = 0; j < n; j++) {
        const uint32_t r = rnd();
        hf[j] = ((r & 1u) ? 0x01u : 0u) | ((r & 2u) ? 0x0100u : 0u) | ((r & 4u) ? 0x010000u : 0u) | ((r & 8u) ? 0x01000000u : 0u);
    }
    for (auto& v : hp) v = (float)((int)(rnd() % 2000001u) - 1000000) * 1.37e-4f * (float)(1u + rnd() % 1000u);
    for (int a = 0, b = 0; a < used; a = b) {
        for (int c = 0; c < GRAD_REC_WORDS; c++) {
            double acc = 0.0;
            for (b = a; b < used && hk[b] == hk[a]; b++)
                for (int q = 0; q < 4; q++)
                    if ((hf[hv[b]] >> (8 * q)) & 0xFFu) acc = acc + (double)hp[((size_t)hv[b] * 4 + q) * DET_SLOT_WORDS + c];
            want[(size_t)hk[a] * GRAD_REC_WORDS + c] = (float)acc;
        }
    }
    uint32_t *dk = nullptr, *dv = nullptr, *df = nullptr;
    float *dp = nullptr, *dg = nullptr;
    uint64_t* dn = nullptr;
    const uint64_t hn = (uint64_t)used;
    int rc = 0;
    if (hipMalloc(&dk, n * 4) != hipSuccess || hipMalloc(&dv, n * 4) != hipSuccess || hipMalloc(&df, n * 4) != hipSuccess ||
        hipMalloc(&dp, hp.size() * 4) != hipSuccess || hipMalloc(&dg, want.size() * 4) != hipSuccess || hipMalloc(&dn, 16) != hipSuccess)
        rc = -1;
    if (rc == 0) {
        std::fill(got.begin(), got.end(), -1.f);   // records of Gaussians without a run are not touched
        (void)hipMemcpyAsync(dk, hk.data(), n * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(dv, hv.data(), n * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(df, hf.data(), n * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(dp, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(dg, got.data(), got.size() * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(dn, &hn, 8, hipMemcpyHostToDevice, stream);
        hipLaunchKernelGGL(k_det_reduce, dim3(37, 1), dim3(256), 0, stream, (const uint32_t*)dk, (const uint32_t*)dv, (const uint32_t*)df,
                           (const float*)dp, (const uint64_t*)dn, (size_t)0, dg, (size_t)0);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(got.data(), dg, got.size() * 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            rc = -1;
    }
    (void)hipFree(dk); (void)hipFree(dv); (void)hipFree(df); (void)hipFree(dp); (void)hipFree(dg); (void)hipFree(dn);
    if (rc != 0) return rc;
    for (size_t j = 0; j < want.size(); j++)
        if (__builtin_memcmp(&got[j], &want[j], 4) != 0) return 1 + (int)j;
    return 0;
}

// ---- the extras' ordered reduction (gsr_backward_batch_channels_det) -------------------------------------------------------------
// The same walk over the same sorted runs as k_det_reduce, on the extra slots xpart[position][quadrant][NX]: lane c < NX of the
// sixteen owns channel c (all sixteen still fetch the run's positions and flag words), adds the marked quadrants 0, 1, 2, 3 of the
// positions in ascending order in a float64 register and rounds once.  Where the view's sum goes: channels [0, n_lo) to
// dst_lo[view][id][c] (rows of n_lo floats, lo_vstride floats per view), channels [n_lo, NX) to dst_hi[view][id][c - n_lo] -- the
// caller's own per-view rows, or the staging of the rows the views share.  Gaussians without a run are not touched.
template <int NX>
__global__ __launch_bounds__(256) void k_det_reduce_x(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                       const uint32_t* __restrict__ flags, const float* __restrict__ xpart,
                                                       const uint64_t* __restrict__ count, size_t d_stride, float* __restrict__ dst_lo,
                                                       size_t lo_vstride, uint32_t n_lo, float* __restrict__ dst_hi, size_t hi_vstride)
{
    const uint32_t view = blockIdx.y;
    key = at_view(key, d_stride, view);
    val = at_view(val, d_stride, view);
    flags = at_view(flags, d_stride, view);
    xpart = at_view(xpart, d_stride, view);
    const uint64_t n = *at_view(count, d_stride, view);
    const uint32_t c = threadIdx.x & 15u, sub = (threadIdx.x >> 4) & 3u;
    const bool mine = c < (uint32_t)NX;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 4); i0 < n; i0 += (uint64_t)gridDim.x * 16u) {
        const uint32_t id = key[i0];
        if (i0 != 0 && key[i0 - 1] == id) continue;   // not the first element of its run
        double acc = 0.0;
        for (uint64_t i = i0;; i += 16u) {
            const uint64_t j = i + c;
            const bool in = j < n && key[j] == id;
            uint32_t pos = 0, f = 0;
            if (in) {
                pos = val[j];
                f = flags[pos];
            }
            const uint32_t cnt = (uint32_t)__popc((uint32_t)(__ballot(in) >> (16u * sub)) & 0xFFFFu);
            for (uint32_t k0 = 0; k0 < cnt; k0 += 8u) {
                float v[8][4];
                uint32_t fk[8];
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
                    const uint32_t pk = (uint32_t)__shfl((int)pos, (int)(k0 + k), 16);
                    // (every lane takes part in the exchange: elements 8..15 of the sixteen sit in lanes that own no channel of eight)
                    const uint32_t fe = (uint32_t)__shfl((int)f, (int)(k0 + k), 16);
                    fk[k] = k0 + k < cnt && mine ? fe : 0u;
                    const float* s = xpart + (size_t)pk * (4 * NX) + c;
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++) v[k][q] = (fk[k] >> (8u * q)) & 0xFFu ? s[q * NX] : 0.f;
                }
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++)
                        if ((fk[k] >> (8u * q)) & 0xFFu) acc += (double)v[k][q];
                }
            }
            if (cnt < 16u) break;
        }
        if (mine) {
            if (c < n_lo) dst_lo[(size_t)view * lo_vstride + (size_t)id * n_lo + c] = (float)acc;
            else dst_hi[(size_t)view * hi_vstride + (size_t)id * ((uint32_t)NX - n_lo) + (c - n_lo)] = (float)acc;
        }
    }
}

// rows the views share: out[i] = the staged per-view sums of element i added for v = 0, 1, .. V - 1 in float64, rounded once
__global__ __launch_bounds__(256) void k_det_viewsum(const float* __restrict__ stage, size_t n, int V, float* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int v = 0; v < V; v++) acc += (double)stage[(size_t)v * n + i];
    out[i] = (float)acc;
}

template <int NX>
static void launch_reduce_x(dim3 grid, hipStream_t stream, const DetView& D, int sorted_buffer, const float* xpart, size_t d_stride,
                            float* dst_lo, size_t lo_vstride, uint32_t n_lo, float* dst_hi, size_t hi_vstride)
{
    hipLaunchKernelGGL(k_det_reduce_x<NX>, grid, dim3(256), 0, stream, (const uint32_t*)D.key[sorted_buffer],
                       (const uint32_t*)D.val[sorted_buffer], (const uint32_t*)D.flags, xpart, (const uint64_t*)D.count, d_stride, dst_lo,
                       lo_vstride, n_lo, dst_hi, hi_vstride);
}

int launch_det_reduce_extra(const Launch& L, const Batch& B, const DetView& D, const float* xpart, size_t d_stride, int sorted_buffer,
                            int P, int nx, int extra_per_view, const ExtraGrads& XG, float* stage)
{
    const size_t n_stage = (size_t)P * (size_t)det_x_shared_channels(nx, extra_per_view);
    // (the caller has cleared `stage`: a Gaussian without a run in a view adds nothing to that view's sum)
    int64_t blocks = div_up(D.cap, 16);
    if (blocks > DET_REDUCE_BLOCKS) blocks = DET_REDUCE_BLOCKS;
    const dim3 grid((unsigned)blocks, B.V);
    // layout 0: every channel staged; 1: every channel into the caller's rows of the view; 2: 0..3 staged, 4..7 into the caller's
    float* lo = extra_per_view == 1 ? XG.grad : stage;
    const size_t lo_vs = extra_per_view == 1 ? (size_t)P * (size_t)nx : n_stage;
    const uint32_t n_lo = extra_per_view == 2 ? 4u : (uint32_t)nx;
    float* hi = extra_per_view == 2 ? XG.grad_hi : nullptr;
    const size_t hi_vs = extra_per_view == 2 ? (size_t)P * 4 : 0;
    if (nx == 4) launch_reduce_x<4>(grid, L.stream, D, sorted_buffer, xpart, d_stride, lo, lo_vs, n_lo, hi, hi_vs);
    else launch_reduce_x<8>(grid, L.stream, D, sorted_buffer, xpart, d_stride, lo, lo_vs, n_lo, hi, hi_vs);
    return check_launch(L, "det_reduce_extra");
}

int launch_det_viewsum(const Launch& L, const Batch& B, int P, int nx, int extra_per_view, const ExtraGrads& XG, const float* stage)
{
    const size_t n_stage = (size_t)P * (size_t)det_x_shared_channels(nx, extra_per_view);
    if (n_stage == 0) return GSR_OK;
    hipLaunchKernelGGL(k_det_viewsum, dim3((unsigned)div_up((int64_t)n_stage, 256)), dim3(256), 0, L.stream, stage, n_stage, B.V, XG.grad);
    return check_launch(L, "det_viewsum");
}

// Self-test of the extras' reduction: random runs, marks and values as in selftest_det_reduce, eight channels in the split layout
// (0..3 staged, 4..7 into per-view rows) and four channels unsplit; then k_det_viewsum over three views of random staged rows.
// The host adds the same floats in the same order.
int selftest_det_reduce_extra(hipStream_t stream)
{
    const int P = 997, n = 20011, V = 3;
    std::vector<uint32_t> hk(n), hv(n), hf(n);
    std::vector<float> hp((size_t)n * 4 * 8), hs((size_t)V * P * 4);
    uint32_t x = 88172645u;
    const auto rnd = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    int used = 0;
    for (uint32_t id = rnd() % 3u; id < (uint32_t)P && used < n; id += 1u + rnd() % 3u) {
        const int len = 1 + (int)(rnd() % 80u);
        for (int j = 0; j < len && used < n; j++) hk[used++] = id;
    }
    for (int j = 0; j < used; j++) hv[j] = (uint32_t)(((uint64_t)j * 7919u) % (uint32_t)n);
    for (int a = 0, b = 0; a < used; a = b) {
        for (b = a; b < used && hk[b] == hk[a];) b++;
        std::sort(hv.begin() + a, hv.begin() + b);
    }
    for (int j = 0; j < n; j++) {
        const uint32_t r = rnd();
        hf[j] = ((r & 1u) ? 0x01u : 0u) | ((r & 2u) ? 0x0100u : 0u) | ((r & 4u) ? 0x010000u : 0u) | ((r & 8u) ? 0x01000000u : 0u);
    }
    const auto val = [&]() { return (float)((int)(rnd() % 2000001u) - 1000000) * 1.37e-4f * (float)(1u + rnd() % 1000u); };
    for (auto& v : hp) v = val();
    for (auto& v : hs) v = val();
    // want8: [P][8] (the test keeps lo and hi rows side by side), want4: [P][4] read from the same block as [n][4][4]; -1 = untouched
    std::vector<float> want8((size_t)P * 8, -1.f), want4((size_t)P * 4, -1.f), wantv((size_t)P * 4);
    for (int a = 0, b = 0; a < used; a = b) {
        for (int nx = 4; nx <= 8; nx += 4)
            for (int c = 0; c < nx; c++) {
                double acc = 0.0;
                for (b = a; b < used && hk[b] == hk[a]; b++)
                    for (int q = 0; q < 4; q++)
                        if ((hf[hv[b]] >> (8 * q)) & 0xFFu) acc = acc + (double)hp[((size_t)hv[b] * 4 + q) * nx + c];
                (nx == 8 ? want8 : want4)[(size_t)hk[a] * nx + c] = (float)acc;
            }
    }
    for (size_t i = 0; i < wantv.size(); i++) {
        double acc = 0.0;
        for (int v = 0; v < V; v++) acc = acc + (double)hs[(size_t)v * wantv.size() + i];
        wantv[i] = (float)acc;
    }
    uint32_t *dk = nullptr, *dv = nullptr, *df = nullptr;
    float *dp = nullptr, *dlo = nullptr, *dhi = nullptr, *d4 = nullptr, *ds = nullptr, *dvs = nullptr;
    uint64_t* dn = nullptr;
    const uint64_t hn = (uint64_t)used;
    const size_t row4 = (size_t)P * 4 * sizeof(float);
    std::vector<float> glo((size_t)P * 4, -1.f), ghi(glo), g4(glo), gv(glo);
    int rc = 0;
    if (hipMalloc(&dk, n * 4) != hipSuccess || hipMalloc(&dv, n * 4) != hipSuccess || hipMalloc(&df, n * 4) != hipSuccess ||
        hipMalloc(&dp, hp.size() * 4) != hipSuccess || hipMalloc(&dlo, row4) != hipSuccess || hipMalloc(&dhi, row4) != hipSuccess ||
        hipMalloc(&d4, row4) != hipSuccess || hipMalloc(&ds, hs.size() * 4) != hipSuccess || hipMalloc(&dvs, row4) != hipSuccess ||
        hipMalloc(&dn, 16) != hipSuccess)
        rc = -1;
    if (rc == 0) {
        (void)hipMemcpyAsync(dk, hk.data(), n * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(dv, hv.data(), n * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(df, hf.data(), n * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(dp, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(ds, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(dn, &hn, 8, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(dlo, glo.data(), row4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(dhi, glo.data(), row4, hipMemcpyHostToDevice, stream);
        (void)hipMemcpyAsync(d4, glo.data(), row4, hipMemcpyHostToDevice, stream);
        DetView D{};
        D.key[0] = dk; D.val[0] = dv; D.flags = df; D.count = dn;
        launch_reduce_x<8>(dim3(37, 1), stream, D, 0, dp, 0, dlo, 0, 4u, dhi, 0);
        launch_reduce_x<4>(dim3(41, 1), stream, D, 0, dp, 0, d4, 0, 4u, nullptr, 0);
        hipLaunchKernelGGL(k_det_viewsum, dim3((unsigned)div_up((int64_t)P * 4, 256)), dim3(256), 0, stream, (const float*)ds,
                           (size_t)P * 4, V, dvs);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(glo.data(), dlo, row4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(ghi.data(), dhi, row4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(g4.data(), d4, row4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(gv.data(), dvs, row4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
            rc = -1;
    }
    (void)hipFree(dk); (void)hipFree(dv); (void)hipFree(df); (void)hipFree(dp); (void)hipFree(dlo); (void)hipFree(dhi); (void)hipFree(d4);
    (void)hipFree(ds); (void)hipFree(dvs); (void)hipFree(dn);
    if (rc != 0) return rc;
    for (int g = 0; g < P; g++)
        for (int c = 0; c < 4; c++) {
            const size_t j = (size_t)g * 4 + c;
            if (__builtin_memcmp(&glo[j], &want8[(size_t)g * 8 + c], 4) != 0) return 1 + (int)j;
            if (__builtin_memcmp(&ghi[j], &want8[(size_t)g * 8 + 4 + c], 4) != 0) return 100001 + (int)j;
            if (__builtin_memcmp(&g4[j], &want4[j], 4) != 0) return 200001 + (int)j;
            if (__builtin_memcmp(&gv[j], &wantv[j], 4) != 0) return 300001 + (int)j;
        }
    return 0;
}

}  // namespace gsr
