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

}  // namespace gsr
