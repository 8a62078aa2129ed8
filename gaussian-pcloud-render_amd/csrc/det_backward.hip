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
// Where the arrays of all this live in the caller's scratch block is DetScratch (common.hpp).  The two reduce kernels keep a copy
// of the walk each: as one inlined function (same additions, bit-identical results) k_det_reduce_x compiled to seven more
// instructions per eight positions and measured 0.8 % slower (profiles/r14_det_reduce_walk.txt).  One fixture and one host sum
// (det_fixture.hpp) check both copies.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "det_fixture.hpp"

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

int launch_det_prepare(const Launch& L, const Batch& B, const DetScratch& S, const uint32_t* point_list, int T)
{
    const DetView& D = S.d;
    hipLaunchKernelGGL(k_det_prefix, dim3(B.V), dim3(1024), 0, L.stream, T, (const uint32_t*)B.iv.tile_need, B.iv_stride, D.slot_base,
                       D.count, S.stride, (uint32_t)D.cap);
    if (int e = check_launch(L, "det_prefix")) return e;
    hipLaunchKernelGGL(k_det_emit, dim3((unsigned)div_up(T, 4), B.V), dim3(256), 0, L.stream, T, (const uint2*)B.iv.ranges, B.iv_stride,
                       point_list, B.b_stride, (const uint32_t*)D.slot_base, D.key[0], D.flags, S.stride, (uint32_t)D.cap);
    return check_launch(L, "det_emit");
}

// key bits of the sort by Gaussian id: ids are < P
static int id_bits(int P)
{
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < (int64_t)P) bits++;
    return bits;
}

int launch_det_sort(const Launch& L, const Batch& B, const DetScratch& S, int P, int* result_buffer)
{
    const DetView& D = S.d;
    const SortJob job{{D.key[0], D.key[1]}, {D.val[0], D.val[1]}, D.hist, D.totals, S.stride, D.count, S.stride, D.cap, B.V};
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

static dim3 reduce_grid(const DetView& D, int V)
{
    const int64_t blocks = div_up(D.cap, 16);
    return dim3((unsigned)(blocks < DET_REDUCE_BLOCKS ? blocks : DET_REDUCE_BLOCKS), V);
}

int launch_det_reduce(const Launch& L, const Batch& B, const DetScratch& S, int sorted_buffer)
{
    const DetView& D = S.d;
    hipLaunchKernelGGL(k_det_reduce, reduce_grid(D, B.V), dim3(256), 0, L.stream, (const uint32_t*)D.key[sorted_buffer],
                       (const uint32_t*)D.val[sorted_buffer], (const uint32_t*)D.flags, (const float*)D.part, (const uint64_t*)D.count,
                       S.stride, B.grad_rec, B.gr_stride);
    return check_launch(L, "det_reduce");
}

template <int NX>
static void launch_reduce_x(dim3 grid, hipStream_t stream, const DetScratch& S, int sorted_buffer, float* dst_lo, size_t lo_vstride,
                            uint32_t n_lo, float* dst_hi, size_t hi_vstride)
{
    const DetView& D = S.d;
    hipLaunchKernelGGL(k_det_reduce_x<NX>, grid, dim3(256), 0, stream, (const uint32_t*)D.key[sorted_buffer],
                       (const uint32_t*)D.val[sorted_buffer], (const uint32_t*)D.flags, (const float*)S.xpart, (const uint64_t*)D.count,
                       S.stride, dst_lo, lo_vstride, n_lo, dst_hi, hi_vstride);
}

int launch_det_reduce_extra(const Launch& L, const Batch& B, const DetScratch& S, int sorted_buffer, int P, int nx, int extra_per_view,
                            const ExtraGrads& XG)
{
    // (the caller has cleared S.stage: a Gaussian without a run in a view adds nothing to that view's sum)
    const dim3 grid = reduce_grid(S.d, B.V);
    // layout 0: every channel staged; 1: every channel into the caller's rows of the view; 2: 0..3 staged, 4..7 into the caller's
    float* lo = extra_per_view == 1 ? XG.grad : S.stage;
    const size_t lo_vs = extra_per_view == 1 ? (size_t)P * (size_t)nx : S.n_stage;
    const uint32_t n_lo = extra_per_view == 2 ? 4u : (uint32_t)nx;
    float* hi = extra_per_view == 2 ? XG.grad_hi : nullptr;
    const size_t hi_vs = extra_per_view == 2 ? (size_t)P * 4 : 0;
    if (nx == 4) launch_reduce_x<4>(grid, L.stream, S, sorted_buffer, lo, lo_vs, n_lo, hi, hi_vs);
    else launch_reduce_x<8>(grid, L.stream, S, sorted_buffer, lo, lo_vs, n_lo, hi, hi_vs);
    return check_launch(L, "det_reduce_extra");
}

int launch_det_viewsum(const Launch& L, const Batch& B, const DetScratch& S, const ExtraGrads& XG)
{
    if (!S.stage) return GSR_OK;
    hipLaunchKernelGGL(k_det_viewsum, dim3((unsigned)div_up((int64_t)S.n_stage, 256)), dim3(256), 0, L.stream, (const float*)S.stage,
                       S.n_stage, B.V, XG.grad);
    return check_launch(L, "det_viewsum");
}

// ---- self-tests --------------------------------------------------------------------------------------------------------------
// The fixture (det_fixture.hpp) on the device, as the single view of a scratch plan: `values` stands for the slots of either kind.
struct DetFixtureDev {
    const uint64_t n = DetFixture::N;
    DevBuf<uint32_t> key, val, flags;
    DevBuf<float> values;
    DevBuf<uint64_t> count;
    DetFixtureDev(const DetFixture& F, hipStream_t s) : key(F.key, s), val(F.val, s), flags(F.flags, s), values(F.values, s), count(1)
    {
        (void)count.upload(&n, s);
    }
    bool ok() const { return key.p && val.p && flags.p && values.p && count.p; }
    DetScratch plan() const
    {
        DetScratch S{};
        S.d.key[0] = key.p; S.d.val[0] = val.p; S.d.flags = flags.p; S.d.count = count.p;
        S.d.part = S.xpart = values.p;
        return S;
    }
};

// 0 when the arrays agree bit for bit, else base + the first index at which they differ
static int first_difference(const std::vector<float>& got, const std::vector<float>& want, int base)
{
    for (size_t j = 0; j < want.size(); j++)
        if (__builtin_memcmp(&got[j], &want[j], 4) != 0) return base + (int)j;
    return 0;
}

// k_det_reduce on the fixture against the host's sums in the same order; records of Gaussians without a run are not touched (-1)
int selftest_det_reduce(hipStream_t stream)
{
    static_assert(GRAD_REC_WORDS == DET_SLOT_WORDS, "a slot is laid out like a record");
    const DetFixture F;
    const std::vector<float> want = F.sums(DET_SLOT_WORDS);
    std::vector<float> got(want.size(), -1.f);
    const DetFixtureDev dev(F, stream);
    const DevBuf<float> rec(got, stream);
    if (!dev.ok() || !rec.p) return -1;
    const DetScratch S = dev.plan();
    hipLaunchKernelGGL(k_det_reduce, dim3(37, 1), dim3(256), 0, stream, (const uint32_t*)S.d.key[0], (const uint32_t*)S.d.val[0],
                       (const uint32_t*)S.d.flags, (const float*)S.d.part, (const uint64_t*)S.d.count, (size_t)0, rec.p, (size_t)0);
    if (hipGetLastError() != hipSuccess || !rec.download(got.data(), stream) || hipStreamSynchronize(stream) != hipSuccess) return -1;
    return first_difference(got, want, 1);
}

// The extras' reduction on the same fixture: eight channels in the split layout (0..3 staged, 4..7 into per-view rows) and four
// channels unsplit; then k_det_viewsum over three views of random staged rows.  The host adds the same floats in the same order.
int selftest_det_reduce_extra(hipStream_t stream)
{
    const int P = DetFixture::P, V = 3;
    DetFixture F;
    const std::vector<float> want8 = F.sums(8), want4 = F.sums(4);
    std::vector<float> wlo((size_t)P * 4), whi(wlo), wantv(wlo), hs((size_t)V * P * 4);   // want8's halves: the rows of channels 0..3 and 4..7
    for (size_t j = 0; j < wlo.size(); j++) {
        wlo[j] = want8[j / 4 * 8 + j % 4];
        whi[j] = want8[j / 4 * 8 + 4 + j % 4];
    }
    for (auto& v : hs) v = F.value();
    for (size_t i = 0; i < wantv.size(); i++) {
        double acc = 0.0;
        for (int v = 0; v < V; v++) acc = acc + (double)hs[(size_t)v * wantv.size() + i];
        wantv[i] = (float)acc;
    }
    std::vector<float> glo((size_t)P * 4, -1.f), ghi(glo), g4(glo), gv(glo);
    const DetFixtureDev dev(F, stream);
    const DevBuf<float> dlo(glo, stream), dhi(glo, stream), d4(glo, stream), ds(hs, stream), dvs(gv.size());
    if (!dev.ok() || !dlo.p || !dhi.p || !d4.p || !ds.p || !dvs.p) return -1;
    const DetScratch S = dev.plan();
    launch_reduce_x<8>(dim3(37, 1), stream, S, 0, dlo.p, 0, 4u, dhi.p, 0);
    launch_reduce_x<4>(dim3(41, 1), stream, S, 0, d4.p, 0, 4u, nullptr, 0);
    hipLaunchKernelGGL(k_det_viewsum, dim3((unsigned)div_up((int64_t)P * 4, 256)), dim3(256), 0, stream, (const float*)ds.p, (size_t)P * 4,
                       V, dvs.p);
    if (hipGetLastError() != hipSuccess || !dlo.download(glo.data(), stream) || !dhi.download(ghi.data(), stream) ||
        !d4.download(g4.data(), stream) || !dvs.download(gv.data(), stream) || hipStreamSynchronize(stream) != hipSuccess)
        return -1;
    if (int r = first_difference(glo, wlo, 1)) return r;
    if (int r = first_difference(ghi, whi, 100001)) return r;
    if (int r = first_difference(g4, want4, 200001)) return r;
    return first_difference(gv, wantv, 300001);
}

}  // namespace gsr
