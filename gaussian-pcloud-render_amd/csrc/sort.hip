// sort.hip -- stable LSD radix sort of (u32 key, u32 value) pairs and the u32 prefix sum.
//
// Role in the pipeline (replaces the reference's CUB calls, CR/rasterizer_impl.cu:277,303-308):
//   the reference sorts R 64-bit keys (tile<<32 | depth bits) with 4-byte payloads in one
//   DeviceRadixSort (6 passes over 12-B pairs at 1080p).  Here the same total order is produced in two
//   steps with 4x less traffic: (1) the P Gaussians are sorted by depth bits (4 passes over P pairs),
//   (2) pairs are emitted in that order and stably sorted by tile id only (ceil(bit/8) passes over R
//   8-B pairs).  Stability of both steps gives exactly: tile, then depth bits, then Gaussian id.
//
// Every launch covers a batch of V independent sort problems (one per camera view, blockIdx.y), laid out at a fixed byte
// stride; a problem's element count may live on the device (the tile sort's num_rendered is never read back mid-frame):
// the grid is sized by the arena capacity and workgroups past the count leave at once.
//
// A pass is three launches -- per-workgroup digit histogram, per-digit row scan, stable scatter: on this part a launch boundary
// is the cheapest device-wide synchronisation there is (the single-launch look-back variant was built,
// measured 2-4x slower and removed, profiles/r06_lookback_sort.txt).
// The scatter ranks keys with wave64 ballots (one ballot per digit bit), reorders the workgroup's 4096
// pairs in LDS, then writes digit runs with consecutive lanes on consecutive addresses.  The key bits
// are split evenly over the passes (13 bits -> 7 + 6, not 8 + 5): narrower digits mean fewer ballots
// and longer, better coalesced runs per workgroup.
#include "block_scan.hpp"
#include "common.hpp"
#include "stats.hpp"

namespace gsr {

struct SortView {
    size_t stride;
    const uint64_t* n_dev;
    size_t n_stride;
    int64_t cap;
    const uint32_t* ctl;   // sortctl of view 0 (depth sort, passes 1..3) or NULL
};
// The depth sort's later passes compare (key - base) and leave at once when their bits are above every difference between two
// keys of visible Gaussians (wave-uniform: one scalar load).  Returns false when the pass has nothing to do.
__device__ __forceinline__ bool pass_control(const SortView& sv, uint32_t view, int shift, uint32_t& base)
{
    base = 0u;
    if (sv.ctl == nullptr) return true;
    const uint32_t* c = at_view(sv.ctl, sv.stride, view);
    base = c[SORTCTL_BASE];
    return (uint32_t)shift < c[SORTCTL_BITS];
}
__device__ __forceinline__ int64_t view_count(const SortView& sv, uint32_t view)
{
    if (sv.n_dev == nullptr) return sv.cap;
    const uint64_t n = *at_view(sv.n_dev, sv.n_stride, view);
    return n < (uint64_t)sv.cap ? (int64_t)n : sv.cap;
}

// ---- pass kernel 1: digit histogram per sort block ------------------------------------------------
// The count matrix is [digit][block], rows padded to whole 64-B lines of HIST_GROUP blocks (k_radix_scatter's workgroup ->
// block map keeps the blocks of one line on one XCD).  Only the digits in use are written.
// (Tried: one histogram workgroup per HIST_GROUP blocks writing whole lines -- the 16 sequential sub-histograms cost more
// than the partial-line stores they save: 61 vs 55 us per launch at 12 views x 11.8 M pairs, 36 vs 11 us for the depth keys.)
constexpr int HIST_GROUP = 16;

template <typename KeyT, int RS_ITEMS>
__global__ __launch_bounds__(RS_THREADS) void k_radix_hist(const KeyT* __restrict__ keys, SortView sv, int shift,
                                                           uint32_t mask, uint32_t* __restrict__ hist, int nblk_pad,
                                                           uint32_t* __restrict__ minmax)   // depth sort, pass 0: [2][nblk_pad], else NULL
{
    constexpr int RS_TILE = RS_THREADS * RS_ITEMS;
    const uint32_t view = blockIdx.y;
    uint32_t kbase;
    if (!pass_control(sv, view, shift, kbase)) return;
    const int64_t n = view_count(sv, view);
    keys = at_view(keys, sv.stride, view);
    hist = at_view(hist, sv.stride, view);
    if (minmax) minmax = at_view(minmax, sv.stride, view);
    const uint32_t d = threadIdx.x;
    if ((int64_t)blockIdx.x * RS_TILE >= n) {   // past the end: this block's column of the count matrix is zero
        if (d <= mask) hist[(size_t)d * nblk_pad + blockIdx.x] = 0;
        if (minmax && d == 0) { minmax[blockIdx.x] = 0xFFFFFFFFu; minmax[nblk_pad + blockIdx.x] = 0u; }
        return;
    }
    // HIST_COPIES private histograms (four per wave, by lane mod 4): same-digit keys of one wave instruction serialise in
    // the LDS atomic unit, the copies quarter those collisions
    constexpr int HIST_COPIES = 4 * RS_WAVES;
    __shared__ __attribute__((aligned(16))) uint32_t h[HIST_COPIES][RADIX];
    __shared__ uint32_t s_min, s_max;
    for (int i = threadIdx.x; i < HIST_COPIES * RADIX / 4; i += RS_THREADS) reinterpret_cast<uint4*>(&h[0][0])[i] = make_uint4(0, 0, 0, 0);
    if (threadIdx.x == 0) { s_min = 0xFFFFFFFFu; s_max = 0u; }
    __syncthreads();
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    const int64_t base = (int64_t)blockIdx.x * RS_TILE;
    const uint32_t w = (threadIdx.x >> 6) * 4u + (threadIdx.x & 3u);
    if (sizeof(KeyT) == 2 && RS_ITEMS % 8 == 0 && base + RS_TILE <= n) {
        // full block of 16-bit keys: 16-B loads of eight keys instead of 2-B ones (counting is order-free)
        const uint4* k4 = reinterpret_cast<const uint4*>(keys + base) + threadIdx.x * (RS_ITEMS / 8);
#pragma unroll
        for (int v = 0; v < RS_ITEMS / 8; v++) {
            const uint4 q = k4[v];
            const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                atomicAdd(&h[w][((wds[j] & 0xFFFFu) >> shift) & mask], 1u);
                atomicAdd(&h[w][((wds[j] >> 16) >> shift) & mask], 1u);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < RS_ITEMS; i++) {
            const int64_t idx = base + i * RS_THREADS + threadIdx.x;
            if (idx < n) {
                const uint32_t key = (uint32_t)keys[idx];
                atomicAdd(&h[w][((key - kbase) >> shift) & mask], 1u);
                if (key != CULLED_KEY) { kmin = key < kmin ? key : kmin; kmax = key > kmax ? key : kmax; }
            }
        }
    }
    if (minmax) {   // (uniform) smallest / largest key of a visible Gaussian in this block
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
            const uint32_t a = __shfl_xor(kmin, dd, 64), b = __shfl_xor(kmax, dd, 64);
            kmin = a < kmin ? a : kmin;
            kmax = b > kmax ? b : kmax;
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&s_min, kmin); atomicMax(&s_max, kmax); }
    }
    __syncthreads();
    if (minmax && d == 0) { minmax[blockIdx.x] = s_min; minmax[nblk_pad + blockIdx.x] = s_max; }
    if (d <= mask) {
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < HIST_COPIES; i++) c += h[i][d];
        hist[(size_t)d * nblk_pad + blockIdx.x] = c;
    }
}

// ---- pass kernel 2: exclusive scan of each digit's row of workgroup counts -----------------------
// Depth sort, pass 0: one more workgroup (blockIdx.x == nrows) reduces the per-block key extremes of the histogram kernel into
// the view's sortctl words -- base = smallest key with its low 8 bits cleared, bits = position of the highest bit in which
// (largest key - base) is set -- so that the passes above `bits` leave at once: depths within a factor of two of each other
// differ in at most 24 bits (one binade = 2^23 codes), and the fourth pass of the 32-bit sort moves nothing.
__global__ __launch_bounds__(256) void k_radix_rowscan(uint32_t* __restrict__ hist, uint32_t* __restrict__ totals, int nblk_pad,
                                                       size_t stride, const uint32_t* __restrict__ ctl, int shift,
                                                       const uint32_t* __restrict__ minmax, uint32_t* __restrict__ ctl_out,
                                                       uint32_t nrows)
{
    __shared__ uint32_t tmp[4];
    if (blockIdx.x == nrows) {
        minmax = at_view(minmax, stride, blockIdx.y);
        uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
        for (int b = threadIdx.x; b < nblk_pad; b += 256) {
            const uint32_t a = minmax[b], c = minmax[nblk_pad + b];
            kmin = a < kmin ? a : kmin;
            kmax = c > kmax ? c : kmax;
        }
        __shared__ uint32_t s_min, s_max;
        if (threadIdx.x == 0) { s_min = 0xFFFFFFFFu; s_max = 0u; }
        __syncthreads();
        atomicMin(&s_min, kmin);
        atomicMax(&s_max, kmax);
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t* c = at_view(ctl_out, stride, blockIdx.y);
            const uint32_t base = s_min <= s_max ? (s_min & ~(uint32_t)(RADIX - 1)) : 0u;
            const uint32_t span = s_min <= s_max ? s_max - base : 0u;      // no visible Gaussian: one pass, any order
            const uint32_t bits = span ? 32u - (uint32_t)__builtin_clz(span) : 0u;
            c[SORTCTL_BASE] = base;
            c[SORTCTL_BITS] = bits < (uint32_t)RADIX_BITS ? (uint32_t)RADIX_BITS : bits;
        }
        return;
    }
    if (ctl != nullptr && (uint32_t)shift >= at_view(ctl, stride, blockIdx.y)[SORTCTL_BITS]) return;
    hist = at_view(hist, stride, blockIdx.y);
    totals = at_view(totals, stride, blockIdx.y);
    uint32_t* row = hist + (size_t)blockIdx.x * nblk_pad;
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nblk_pad; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const uint32_t v = b < nblk_pad ? row[b] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan_256(v, tmp, &tot);
        if (b < nblk_pad) row[b] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

#ifdef GSR_STATS
// instrumentation build only: per-phase time of the scatter workgroups of the LAST launch (one record per workgroup, 10-ns ticks):
// 0 keys/values loaded, 1 ranking, 2 prefix sums, 3 reorder in LDS, 4 stores issued
constexpr int SC_REC = 65536;
__device__ unsigned g_sc_rec[SC_REC][5];
// phase i of the calling workgroup's record
__device__ __forceinline__ void scatter_record(int i, unsigned long long ticks)
{
    const unsigned r = blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0 && r < SC_REC) g_sc_rec[r][i] = (unsigned)ticks;
}
// out8[0..4]: the phases summed over the workgroups that ran, out8[5]: how many did
int debug_scatter_times(unsigned long long* out8, int reset)
{
    const auto host = read_wave_records(g_sc_rec, reset);
    if (!host) return -1;
    for (int i = 0; i < 8; i++) out8[i] = 0;
    for (int r = 0; r < SC_REC; r++) {
        if (host[r][1] == 0) continue;
        for (int i = 0; i < 5; i++) out8[i] += host[r][i];
        out8[5]++;
    }
    return 0;
}
#endif

// ---- pass kernel 3: stable scatter ----------------------------------------------------------------
// The block's per-digit offsets come from the count matrix the row scan left (hist / totals).
template <int BITS, typename KeyT, int RS_ITEMS>
__global__ __launch_bounds__(RS_THREADS) void k_radix_scatter(const KeyT* __restrict__ keys_in,
                                                              const uint32_t* __restrict__ vals_in,  // NULL: value = index
                                                              KeyT* __restrict__ keys_out,
                                                              uint32_t* __restrict__ vals_out, SortView sv, int shift,
                                                              uint32_t mask, const uint32_t* __restrict__ hist,
                                                              const uint32_t* __restrict__ totals, int nblk_pad)
{
    constexpr int RS_TILE = RS_THREADS * RS_ITEMS;
    const uint32_t view = blockIdx.y;
    uint32_t kbase;
    if (!pass_control(sv, view, shift, kbase)) return;
    const int64_t n = view_count(sv, view);
    // Workgroup -> sort block: the HIST_GROUP blocks whose counters share a 64-B line of the count matrix run on ONE XCD
    // (workgroup w runs on XCD w % 8), so the line is fetched into that L2 once instead of by sixteen different L2s.
    const uint32_t wg = blockIdx.x, xcd = wg & 7u, r = wg >> 3;
    const uint32_t blk = ((r / HIST_GROUP) * 8u + xcd) * HIST_GROUP + (r % HIST_GROUP);
    hist = at_view(hist, sv.stride, view);
    totals = at_view(totals, sv.stride, view);
    if ((int64_t)blk * RS_TILE >= n) return;
    keys_in = at_view(keys_in, sv.stride, view);
    if (vals_in) vals_in = at_view(vals_in, sv.stride, view);
    keys_out = at_view(keys_out, sv.stride, view);
    vals_out = at_view(vals_out, sv.stride, view);
    __shared__ uint32_t s_key[RS_TILE];
    __shared__ uint32_t s_val[RS_TILE];
    __shared__ uint32_t wave_cnt[RS_WAVES][RADIX];  // running per-wave digit counts, then exclusive over waves
    __shared__ uint32_t local_base[RADIX];          // first slot of digit d inside this workgroup's sorted tile
    __shared__ uint32_t global_base[RADIX];         // first global slot of this workgroup's digit-d run
    __shared__ uint32_t tmp[4];

    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t blk_base = (int64_t)blk * RS_TILE;
    const int64_t seg_base = blk_base + (int64_t)w * (RS_TILE / RS_WAVES);

    for (int i = lane; i < RADIX; i += 64) wave_cnt[w][i] = 0;
    WALK_T(t0);

    // requested before the keys (loads return in order): see gbase_d below
    const uint32_t tot_d = tid <= mask ? totals[tid] : 0u;
    const uint32_t hist_d = tid <= mask ? hist[(size_t)tid * nblk_pad + blk] : 0u;

    uint32_t k[RS_ITEMS], v[RS_ITEMS], rank[RS_ITEMS];
    const bool full = blk_base + RS_TILE <= n;   // all but the last block of a view: no bounds checks
    {
        const KeyT* kp = keys_in + seg_base + lane;
        const uint32_t* vp = vals_in ? vals_in + seg_base + lane : nullptr;
        // keys are ranked (and staged) as key - kbase; kbase goes back on when they are written (kbase = 0 but in the depth sort)
        if (full) {
#pragma unroll
            for (int j = 0; j < RS_ITEMS; j++) k[j] = (uint32_t)kp[j * 64] - kbase;
            if (vp) {
#pragma unroll
                for (int j = 0; j < RS_ITEMS; j++) v[j] = vp[j * 64];
            } else {
#pragma unroll
                for (int j = 0; j < RS_ITEMS; j++) v[j] = (uint32_t)(seg_base + j * 64 + lane);
            }
        } else {
#pragma unroll
            for (int j = 0; j < RS_ITEMS; j++) {
                const int64_t idx = seg_base + j * 64 + lane;
                const bool ok = idx < n;
                k[j] = ok ? (uint32_t)kp[j * 64] - kbase : 0xFFFFFFFFu;
                v[j] = ok ? (vp ? vp[j * 64] : (uint32_t)idx) : 0u;
            }
        }
    }
    // digit d = tid: first global slot of this workgroup's digit-d run = digits below d in the whole array + digit d in the
    // blocks before this one.  Needs nothing from the keys: the two loads and the scan overlap the key loads' latency instead
    // of sitting between ranking and reorder (a fifth of the workgroup's life there, scripts/dup_times.py).
    uint32_t gbase_d = block_exclusive_scan_256(tot_d, tmp, nullptr) + hist_d;
    __builtin_amdgcn_wave_barrier();
    WALK_STAT(asm volatile("s_waitcnt vmcnt(0)" ::: "memory");)   // (the loads belong to the phase that issued them)
    WALK_T(t1);
    WALK_STAT(scatter_record(0, t1 - t0);)

    // stable rank inside the wave's segment: order is (j, lane).  peers = the lanes holding my digit: one ballot per digit
    // bit, folded in with one three-input bit operation per half (peers & ~(ballot ^ my bit)); the count of peers below me
    // comes from mbcnt.  This loop is most of the kernel's instructions -- the scatter is VALU-bound, not HBM-bound.
#pragma unroll
    for (int j = 0; j < RS_ITEMS; j++) {
        const bool ok = full || seg_base + j * 64 + lane < n;
        const uint32_t d = (k[j] >> shift) & mask;
        const uint64_t okb = full ? ~0ull : __ballot(ok);
        uint32_t plo = (uint32_t)okb, phi = (uint32_t)(okb >> 32);
#pragma unroll
        for (int b = 0; b < BITS; b++) {
            const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int32_t)k[j], (uint32_t)(shift + b), 1u);   // all ones where my bit b is set
            const uint64_t bal = __ballot(m != 0u);
            plo = __builtin_amdgcn_bitop3_b32(plo, (uint32_t)bal, m, 0x90);          // a & ~(b ^ c)
            phi = __builtin_amdgcn_bitop3_b32(phi, (uint32_t)(bal >> 32), m, 0x90);
        }
        const uint32_t before = wave_cnt[w][d];
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
        rank[j] = before + below;
        __builtin_amdgcn_wave_barrier();
        if (ok && below == 0) wave_cnt[w][d] = before + (uint32_t)__popc(plo) + (uint32_t)__popc(phi);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    WALK_T(t2);
    WALK_STAT(scatter_record(1, t2 - t1);)

    // digit d = tid: exclusive prefix over waves, workgroup-local and global run starts
    {
        const uint32_t d = tid;
        uint32_t c[RS_WAVES], run = 0;
#pragma unroll
        for (int i = 0; i < RS_WAVES; i++) {
            c[i] = wave_cnt[i][d];
            wave_cnt[i][d] = run;
            run += c[i];
        }
        const uint32_t lbase = block_exclusive_scan_256(run, tmp, nullptr);
        local_base[d] = lbase;
        global_base[d] = gbase_d;
    }
    __syncthreads();
    WALK_T(t3);
    WALK_STAT(scatter_record(2, t3 - t2);)

#pragma unroll
    for (int j = 0; j < RS_ITEMS; j++) {
        if (full || seg_base + j * 64 + lane < n) {
            const uint32_t d = (k[j] >> shift) & mask;
            const uint32_t pos = local_base[d] + wave_cnt[w][d] + rank[j];
            s_key[pos] = k[j];
            s_val[pos] = v[j];
        }
    }
    __syncthreads();
    WALK_T(t4);
    WALK_STAT(scatter_record(3, t4 - t3);)

    const int64_t rem = n - blk_base;
    const uint32_t count = rem < RS_TILE ? (uint32_t)rem : (uint32_t)RS_TILE;
#pragma unroll
    for (int i = 0; i < RS_ITEMS; i++) {
        const uint32_t p = i * RS_THREADS + tid;
        if (p < count) {
            const uint32_t key = s_key[p];
            const uint32_t d = (key >> shift) & mask;
            const size_t g = (size_t)global_base[d] + (p - local_base[d]);
            keys_out[g] = (KeyT)(key + kbase);
            vals_out[g] = s_val[p];
        }
    }
    WALK_STAT({ WALK_T(t5); scatter_record(4, t5 - t4); })
}

// Sorts on key bits [0, end_bit).  job.key[0]/val[0] hold the input (val[0] ignored when iota_vals); the
// result lands in key[*result_buffer] / val[*result_buffer] (the parity only depends on end_bit).
int launch_radix_sort_pairs(const Launch& L, const SortJob& job, bool iota_vals, int end_bit, int* result_buffer, bool key16)
{
    int cur = 0;
    if (job.cap > 0 && job.V > 0) {
        const bool small = job.small_blocks && !key16 && end_bit % RADIX_BITS == 0;   // (every digit 8 bits wide)
        const int tile = small ? RS_TILE_SMALL : RS_TILE;
        const int nblk = (int)div_up(job.cap, tile);
        const int nblk_pad = sort_hist_stride(job.cap, tile);
        SortView sv{job.stride, job.n_dev, job.n_stride, job.cap, nullptr};
        const dim3 grid_hist(nblk_pad, job.V);
        const dim3 grid((unsigned)div_up(nblk, 8 * HIST_GROUP) * 8 * HIST_GROUP, job.V);   // see the workgroup -> block map
        bool first = true;
        const int npass = (end_bit + RADIX_BITS - 1) / RADIX_BITS;
        int shift = 0;
        for (int pass = 0; pass < npass; pass++) {
            const int bits = (end_bit - shift + (npass - pass) - 1) / (npass - pass);   // even split, wider digits first
            const uint32_t mask = (1u << bits) - 1u;
            // depth sort: pass 0 produces the control words, the later passes obey them
            const bool make_ctl = job.sortctl != nullptr && pass == 0;
            sv.ctl = (job.sortctl != nullptr && pass > 0) ? job.sortctl : nullptr;
            uint32_t* minmax = make_ctl ? job.blk_minmax : nullptr;
            if (key16)
                hipLaunchKernelGGL((k_radix_hist<uint16_t, RS_ITEMS>), grid_hist, dim3(RS_THREADS), 0, L.stream, (const uint16_t*)job.key[cur], sv,
                                   shift, mask, job.hist, nblk_pad, minmax);
            else if (small)
                hipLaunchKernelGGL((k_radix_hist<uint32_t, RS_ITEMS_SMALL>), grid_hist, dim3(RS_THREADS), 0, L.stream, (const uint32_t*)job.key[cur], sv,
                                   shift, mask, job.hist, nblk_pad, minmax);
            else
                hipLaunchKernelGGL((k_radix_hist<uint32_t, RS_ITEMS>), grid_hist, dim3(RS_THREADS), 0, L.stream, (const uint32_t*)job.key[cur], sv,
                                   shift, mask, job.hist, nblk_pad, minmax);
            if (int e = check_launch(L, "radix_hist")) return e;
            hipLaunchKernelGGL(k_radix_rowscan, dim3(mask + 1u + (make_ctl ? 1u : 0u), job.V), dim3(256), 0, L.stream, job.hist,
                               job.totals, nblk_pad, job.stride, sv.ctl, shift, (const uint32_t*)minmax, job.sortctl, mask + 1u);
            if (int e = check_launch(L, "radix_rowscan")) return e;
            const uint32_t* vin = (first && iota_vals) ? (const uint32_t*)nullptr : (const uint32_t*)job.val[cur];
#define GSR_SCATTER(B)                                                                                                        \
    case B:                                                                                                                   \
        if (key16)                                                                                                            \
            hipLaunchKernelGGL((k_radix_scatter<B, uint16_t, RS_ITEMS>), grid, dim3(RS_THREADS), 0, L.stream,                 \
                               (const uint16_t*)job.key[cur], vin, (uint16_t*)job.key[cur ^ 1], job.val[cur ^ 1], sv, shift,  \
                               mask, job.hist, job.totals, nblk_pad);                                                         \
        else                                                                                                                  \
            hipLaunchKernelGGL((k_radix_scatter<B, uint32_t, RS_ITEMS>), grid, dim3(RS_THREADS), 0, L.stream,                 \
                               (const uint32_t*)job.key[cur], vin, job.key[cur ^ 1], job.val[cur ^ 1], sv, shift, mask,       \
                               job.hist, job.totals, nblk_pad);                                                               \
        break;
            if (small)
                hipLaunchKernelGGL((k_radix_scatter<RADIX_BITS, uint32_t, RS_ITEMS_SMALL>), grid, dim3(RS_THREADS), 0, L.stream,
                                   (const uint32_t*)job.key[cur], vin, job.key[cur ^ 1], job.val[cur ^ 1], sv, shift, mask, job.hist,
                                   job.totals, nblk_pad);
            else switch (bits) {
                GSR_SCATTER(1) GSR_SCATTER(2) GSR_SCATTER(3) GSR_SCATTER(4) GSR_SCATTER(5) GSR_SCATTER(6) GSR_SCATTER(7)
                GSR_SCATTER(8)
            }
#undef GSR_SCATTER
            if (int e = check_launch(L, "radix_scatter")) return e;
            cur ^= 1;
            first = false;
            shift += bits;
        }
    } else {
        cur = ((end_bit + RADIX_BITS - 1) / RADIX_BITS) & 1;
    }
    *result_buffer = cur;
    return GSR_OK;
}

}  // namespace gsr
