// inspect.hip -- the entries of include/gsr.h that only tests, the bench's roofline report and the instrumentation scripts call: reads of
// the arenas (gsr_query), the clock probe, the device self-test, the probes of sort.hip and binning.hip, the per-step timing's switch
// and read-out, and the exports of the instrumentation build.  The render path (api.hip) calls nothing in here.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "host.hpp"

using namespace gsr;

extern "C" {

namespace {
// One wave reads the shader clock (s_memtime: one tick per shader cycle) and the constant-rate wall clock (s_memrealtime) around a
// fixed chain of dependent FMAs: delta(shader) / delta(wall) x the wall clock rate is the shader clock the chip is running at
// while the probe is resident -- next to whatever else is on the device (DVFS follows the power budget, so a kernel time means
// little without the clock it was measured at).
__global__ void k_clock_probe(unsigned long long* out, int iters)
{
    const unsigned long long s0 = clock64(), w0 = wall_clock64();
    float x = (float)threadIdx.x * 1e-3f;
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int k = 0; k < 64; k++) x = __builtin_fmaf(x, 0.999f, 1e-3f);
    }
    const unsigned long long s1 = clock64(), w1 = wall_clock64();
    if (threadIdx.x == 0) {
        out[0] = s1 - s0;
        out[1] = w1 - w0;
    }
    if (x == 12345.678f) out[1] = 0;   // keeps the chain
}
__global__ void k_query(int what, int64_t n, const Splat* __restrict__ sp, const uint8_t* __restrict__ clamped,
                        const uint32_t* __restrict__ k, int key16, const uint32_t* __restrict__ v, void* __restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float* d = (float*)dst;
    switch (what) {
    case GSR_Q_DEPTHS: d[i] = sp[i].q2.y; break;
    case GSR_Q_MEANS2D: d[2 * i] = sp[i].q0.x; d[2 * i + 1] = sp[i].q0.y; break;
    case GSR_Q_CONIC_OPACITY:
        d[4 * i] = sp[i].q0.z; d[4 * i + 1] = sp[i].q0.w; d[4 * i + 2] = sp[i].q1.x; d[4 * i + 3] = sp[i].q1.y;
        break;
    case GSR_Q_RGB: d[3 * i] = sp[i].q1.z; d[3 * i + 1] = sp[i].q1.w; d[3 * i + 2] = sp[i].q2.x; break;
    case GSR_Q_POINT_LIST_KEYS:
        ((uint64_t*)dst)[i] = ((uint64_t)(key16 ? (uint32_t)((const uint16_t*)k)[i] : k[i]) << 32) | (uint64_t)__float_as_uint(sp[v[i]].q2.y);
        break;
    case GSR_Q_LIST_PAIRS: {
        const uint64_t* c = (const uint64_t*)k;   // k = the view's counters
        if (i == 0) { ((uint64_t*)dst)[0] = c[CNT_NUM_RENDERED]; ((uint64_t*)dst)[1] = c[CNT_NUM_REFERENCE]; }
        break;
    }
    case GSR_Q_DEPTH_SORT: {
        uint32_t* o = (uint32_t*)dst;   // k = the view's sortctl words
        if (i == 0) { o[0] = k[SORTCTL_BASE]; o[1] = k[SORTCTL_BITS]; o[2] = depth_sort_passes(k[SORTCTL_BITS]); o[3] = 0u; }
        break;
    }
    case GSR_Q_CLAMPED: {
        uint8_t* c = (uint8_t*)dst;
        c[3 * i] = clamped[i] & 1; c[3 * i + 1] = (clamped[i] >> 1) & 1; c[3 * i + 2] = (clamped[i] >> 2) & 1;
        break;
    }
    default: break;
    }
}
}  // namespace

int gsr_query(const gsr_params* p, int what, const void* geom, const void* binning, size_t binning_bytes, const void* image,
              int64_t R, void* dst, size_t dst_bytes, gsr_stream_t stream)
{
    if (!p || !dst) return fail(GSR_ERR_INVALID, "[gsr] query: NULL");
    hipStream_t s = (hipStream_t)stream;
    const int P = p->P, T = tile_count(p);
    const int64_t N = (int64_t)p->W * p->H;
    const GeomView g = geom_view(align256(const_cast<void*>(geom)), P);
    if (binning && binning_bytes < 512) return fail(GSR_ERR_CAPACITY, "[gsr] query: binning arena too small");
    const int64_t cap = binning ? bin_capacity_from_bytes(((binning_bytes - 256)) / 256 * 256) : 0;
    if (binning && R > cap && (what == GSR_Q_POINT_LIST || what == GSR_Q_POINT_LIST_KEYS))
        return fail(GSR_ERR_CAPACITY, "[gsr] query: arena holds %lld pairs, asked for %lld (the lists hold GSR_Q_LIST_PAIRS pairs)", (long long)cap, (long long)R);
    const BinView b = bin_view(align256(const_cast<void*>(binning)), cap > 0 ? cap : 1);
    const ImageView iv = image_view(align256(const_cast<void*>(image)), p->W, p->H);
    const int res = sorted_buffer(T);
    int64_t n = 0;
    size_t bytes = 0;
    const void* src = nullptr;
    switch (what) {
    case GSR_Q_DEPTHS: n = P; bytes = (size_t)P * 4; break;
    case GSR_Q_MEANS2D: n = P; bytes = (size_t)P * 8; break;
    case GSR_Q_CONIC_OPACITY: n = P; bytes = (size_t)P * 16; break;
    case GSR_Q_RGB: n = P; bytes = (size_t)P * 12; break;
    case GSR_Q_CLAMPED: n = P; bytes = (size_t)P * 3; break;
    case GSR_Q_POINT_LIST_KEYS: n = R; bytes = (size_t)R * 8; break;
    case GSR_Q_TILES_TOUCHED: src = g.tiles_touched; bytes = (size_t)P * 4; break;
    case GSR_Q_POINT_LIST: src = b.val[res]; bytes = (size_t)R * 4; break;
    case GSR_Q_RANGES: src = iv.ranges; bytes = (size_t)T * 8; break;
    case GSR_Q_FINAL_T: src = iv.final_T; bytes = (size_t)N * 4; break;
    case GSR_Q_N_CONTRIB: src = iv.n_contrib; bytes = (size_t)N * 4; break;
    case GSR_Q_TILE_NEED: src = iv.tile_need; bytes = (size_t)T * 4; break;
    case GSR_Q_DEPTH_SORT: n = 1; bytes = 16; break;
    case GSR_Q_LIST_PAIRS: n = 1; bytes = 16; break;
    default: return fail(GSR_ERR_INVALID, "[gsr] query: unknown item %d", what);
    }
    if (dst_bytes < bytes) return fail(GSR_ERR_CAPACITY, "[gsr] query %d: destination too small", what);
    if (bytes == 0) return GSR_OK;
    if (src) {
        if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(GSR_ERR_HIP, "[gsr] query copy failed");
    } else {
        hipLaunchKernelGGL(k_query, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, what, n, g.splat, g.clamped,
                           what == GSR_Q_DEPTH_SORT ? (const uint32_t*)g.sortctl
                           : what == GSR_Q_LIST_PAIRS ? (const uint32_t*)g.counters : (const uint32_t*)b.key[res],
                           (int)tile_keys16(T), b.val[res], dst);
        if (hipGetLastError() != hipSuccess) return fail(GSR_ERR_HIP, "[gsr] query kernel failed");
    }
    return GSR_OK;
}

// Device self-test of internal primitives that have no observable output of their own: the matrix-core pixel
// contraction of the render backward, and the stable radix sort against std::stable_sort on random keys with many ties.
int gsr_selftest(gsr_stream_t stream)
{
    hipStream_t s = (hipStream_t)stream;
    const DevBuf<float> d(256);
    if (!d.p) return fail(GSR_ERR_HIP, "[gsr] selftest: hipMalloc failed");
    const int rm = selftest_mm(s, d.p);
    if (rm != 0) return fail(GSR_ERR_HIP, "[gsr] selftest: matrix-core pixel contraction wrong at check %d", rm);
    const int rd = selftest_det_reduce(s);
    if (rd != 0) return fail(GSR_ERR_HIP, "[gsr] selftest: ordered reduction of the deterministic backward differs from the host sum at check %d", rd);
    const int rx = selftest_det_reduce_extra(s);
    if (rx != 0) return fail(GSR_ERR_HIP, "[gsr] selftest: ordered reduction of the extra channels differs from the host sum at check %d", rx);

    const int64_t n = 100003;
    std::vector<uint32_t> hk(n), hv(n), order(n);
    uint32_t x = 12345u;
    for (int64_t i = 0; i < n; i++) {
        x = x * 1664525u + 1013904223u;
        hk[i] = (x >> 8) % 3001u;  // many ties
        hv[i] = (uint32_t)i;
        order[i] = (uint32_t)i;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hk[a] < hk[b]; });
    const DevBuf<uint32_t> k0(hk, s), k1(n), v0(n), v1(n), hist(RADIX * (size_t)sort_hist_stride(n)), tot(RADIX);
    if (!k0.p || !k1.p || !v0.p || !v1.p || !hist.p || !tot.p) return fail(GSR_ERR_HIP, "[gsr] selftest: hipMalloc failed");
    int res = 0;
    const Launch L{s, 1};
    const SortJob job{{k0.p, k1.p}, {v0.p, v1.p}, hist.p, tot.p, 0, nullptr, 0, n, 1};
    if (int rc = launch_radix_sort_pairs(L, job, /*iota_vals=*/true, 12, &res)) return rc;
    std::vector<uint32_t> gk(n), gv(n);
    if (!(res ? k1 : k0).download(gk.data(), s) || !(res ? v1 : v0).download(gv.data(), s) || hipStreamSynchronize(s) != hipSuccess)
        return GSR_ERR_HIP;
    for (int64_t i = 0; i < n; i++)
        if (gv[i] != order[i] || gk[i] != hk[order[i]]) return fail(GSR_ERR_HIP, "[gsr] selftest: radix sort differs from std::stable_sort at %lld", (long long)i);
    return GSR_OK;
}

// Test probe of sort.hip: launch_radix_sort_pairs on the caller's arrays, in work buffers of its own (freed on every path, like the
// self-test's).  The caller says which kernels run (key width, block size, depth control); nothing is decided silently here.
int gsr_sort_probe(const void* keys, const uint32_t* vals, size_t stride, const uint64_t* n_dev, size_t n_stride, int V, int64_t cap,
                   int end_bit, int flags, void* keys_out, uint32_t* vals_out, uint32_t* ctl_out, gsr_stream_t stream)
{
    const bool key16 = (flags & GSR_SORT_KEY16) != 0, small = (flags & GSR_SORT_SMALL_BLOCKS) != 0, depth = (flags & GSR_SORT_DEPTH_CTL) != 0;
    if (flags & ~(GSR_SORT_KEY16 | GSR_SORT_SMALL_BLOCKS | GSR_SORT_DEPTH_CTL)) return fail(GSR_ERR_INVALID, "[gsr] sort probe: unknown flags 0x%x", flags);
    if (!keys || !keys_out || !vals_out) return fail(GSR_ERR_INVALID, "[gsr] sort probe: NULL keys or outputs");
    if (V < 1) return fail(GSR_ERR_INVALID, "[gsr] sort probe: view count %d", V);
    if (cap < 0 || cap > ((int64_t)1 << 30)) return fail(GSR_ERR_INVALID, "[gsr] sort probe: capacity %lld", (long long)cap);
    if (end_bit < 1 || end_bit > 32) return fail(GSR_ERR_INVALID, "[gsr] sort probe: end_bit %d is not in 1..32", end_bit);
    if (key16 && end_bit > 16) return fail(GSR_ERR_INVALID, "[gsr] sort probe: 16-bit keys have no bit %d", end_bit - 1);
    if (depth && (end_bit != 32 || key16 || vals != nullptr))
        return fail(GSR_ERR_INVALID, "[gsr] sort probe: depth control sorts 32 bits of uint32_t keys with index values");
    if (depth && !ctl_out) return fail(GSR_ERR_INVALID, "[gsr] sort probe: depth control needs ctl_out");
    if (small && (key16 || end_bit % RADIX_BITS != 0))
        return fail(GSR_ERR_INVALID, "[gsr] sort probe: small blocks take uint32_t keys and whole 8-bit digits");
    const size_t ksz = key16 ? 2 : 4;
    if (V > 1 && (stride % 256 != 0 || stride < (size_t)cap * 4))
        return fail(GSR_ERR_INVALID, "[gsr] sort probe: view stride %zu (a multiple of 256, at least 4 * cap)", stride);
    if (n_dev && V > 1 && (n_stride == 0 || n_stride % 8 != 0)) return fail(GSR_ERR_INVALID, "[gsr] sort probe: count stride %zu", n_stride);
    if (cap == 0) return GSR_OK;

    hipStream_t s = (hipStream_t)stream;
    const int tile = small ? RS_TILE_SMALL : RS_TILE;
    const size_t nblk_pad = (size_t)sort_hist_stride(cap, tile);
    // one stride serves every array of a SortJob: the caller's when the count matrix fits it (the views then sit at the caller's
    // alignment), else the count matrix's size
    const size_t need = std::max(align_up((size_t)cap * 4, 256), (size_t)RADIX * nblk_pad * 4);
    const size_t S = (V > 1 && stride >= need) ? stride : need;
    const size_t words = (size_t)V * S / 4;
    const DevBuf<uint32_t> k0(words), k1(words), v0(words), v1(words), hist(words), tot(words), mm(words), ctl(words);
    if (!k0.p || !k1.p || !v0.p || !v1.p || !hist.p || !tot.p || !mm.p || !ctl.p) return fail(GSR_ERR_HIP, "[gsr] sort probe: hipMalloc failed");
    const auto hip_fail = [&](const char* what) {
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        return fail(GSR_ERR_HIP, "[gsr] sort probe: %s failed", what);
    };
    if (hipMemsetAsync(ctl.p, 0, words * 4, s) != hipSuccess) return hip_fail("memset");
    for (int v = 0; v < V; v++) {
        if (hipMemcpyAsync((char*)k0.p + v * S, (const char*)keys + v * stride, (size_t)cap * ksz, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            (vals && hipMemcpyAsync((char*)v0.p + v * S, (const char*)vals + v * stride, (size_t)cap * 4, hipMemcpyDeviceToDevice, s) != hipSuccess))
            return hip_fail("copy in");
    }
    SortJob job{{k0.p, k1.p}, {v0.p, v1.p}, hist.p, tot.p, S, n_dev, n_stride, cap, V};
    job.small_blocks = small;
    if (depth) { job.blk_minmax = mm.p; job.sortctl = ctl.p; }
    int res = 0;
    const Launch L{s, 1};
    if (int rc = launch_radix_sort_pairs(L, job, /*iota_vals=*/vals == nullptr, end_bit, &res, key16)) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    std::vector<uint32_t> hctl((size_t)V * 4, 0u);
    if (depth) {
        for (int v = 0; v < V; v++)
            if (hipMemcpyAsync(&hctl[4 * (size_t)v], (const char*)ctl.p + v * S, 16, hipMemcpyDeviceToHost, s) != hipSuccess) return hip_fail("control words");
        if (hipStreamSynchronize(s) != hipSuccess) return hip_fail("sort");
    }
    for (int v = 0; v < V; v++) {
        int buf = res;
        if (depth) {   // (base, bits, passes, 0) like GSR_Q_DEPTH_SORT; a view's result is where ITS pass count left it
            hctl[4 * (size_t)v + 2] = depth_sort_passes(hctl[4 * (size_t)v + SORTCTL_BITS]);
            hctl[4 * (size_t)v + 3] = 0u;
            buf = (int)(hctl[4 * (size_t)v + 2] & 1u);
        }
        if (hipMemcpyAsync((char*)keys_out + v * stride, (const char*)job.key[buf] + v * S, (size_t)cap * ksz, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync((char*)vals_out + v * stride, (const char*)job.val[buf] + v * S, (size_t)cap * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return hip_fail("copy out");
    }
    if (depth && hipMemcpyAsync(ctl_out, hctl.data(), (size_t)V * 16, hipMemcpyHostToDevice, s) != hipSuccess) return hip_fail("control words");
    if (hipStreamSynchronize(s) != hipSuccess) return hip_fail("sort");
    return GSR_OK;
}

// Test probe of binning.hip: k_tile_ranges on the caller's sorted keys and device counts, straight into the caller's ranges.
int gsr_tile_ranges_probe(const void* keys, size_t stride, const uint64_t* n_dev, size_t n_stride, int V, int64_t cap, int T, int key16,
                          uint32_t* ranges, gsr_stream_t stream)
{
    if (!keys || !n_dev || !ranges) return fail(GSR_ERR_INVALID, "[gsr] tile ranges probe: NULL");
    if (V < 1) return fail(GSR_ERR_INVALID, "[gsr] tile ranges probe: view count %d", V);
    if (cap < 0 || cap > 0xFFFFFFFFll) return fail(GSR_ERR_INVALID, "[gsr] tile ranges probe: capacity %lld", (long long)cap);
    if (T < 1 || (key16 && T > 65536)) return fail(GSR_ERR_INVALID, "[gsr] tile ranges probe: %d tiles", T);
    if (V > 1 && (stride % 16 != 0 || stride < (size_t)cap * (key16 ? 2 : 4) || n_stride == 0 || n_stride % 8 != 0))
        return fail(GSR_ERR_INVALID, "[gsr] tile ranges probe: view strides %zu / %zu", stride, n_stride);
    hipStream_t s = (hipStream_t)stream;
    const Launch L{s, 1};
    if (int rc = launch_tile_ranges_raw(L, V, n_dev, n_stride, cap, keys, stride, reinterpret_cast<uint2*>(ranges), (size_t)T * sizeof(uint2), T, key16 != 0)) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    return GSR_OK;
}

int gsr_clock_probe_launch(void* dst16, int iters, gsr_stream_t stream)
{
    if (!dst16 || iters < 1) return fail(GSR_ERR_INVALID, "[gsr] clock probe: bad argument");
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)dst16, iters);
    if (hipGetLastError() != hipSuccess) return fail(GSR_ERR_HIP, "[gsr] clock probe launch failed");
    return GSR_OK;
}

int gsr_wall_clock_khz(void)
{
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 0;
    return khz;
}

void gsr_set_profiling(int on) { gsr::set_profiling(on); }
int gsr_get_profile(const char** names, float* ms, int cap) { return gsr::get_profile(names, ms, cap); }

#ifdef GSR_STATS
__attribute__((visibility("default"))) int gsr_debug_bwd_stats(unsigned long long* out8, int reset) { return gsr::debug_bwd_stats(out8, reset); }
__attribute__((visibility("default"))) int gsr_debug_scatter_times(unsigned long long* out8, int reset) { return gsr::debug_scatter_times(out8, reset); }
__attribute__((visibility("default"))) int gsr_debug_fwd_times(unsigned long long* out8, int reset) { return gsr::debug_fwd_times(out8, reset); }
__attribute__((visibility("default"))) int gsr_debug_fwd_records(unsigned* out, int n) { return gsr::debug_fwd_records(out, n); }
__attribute__((visibility("default"))) int gsr_debug_bwd_times(unsigned long long* out8, int reset) { return gsr::debug_bwd_times(out8, reset); }
__attribute__((visibility("default"))) int gsr_debug_bwd_records(unsigned* out, int n) { return gsr::debug_bwd_records(out, n); }
__attribute__((visibility("default"))) int gsr_debug_dup_times(unsigned long long* out8, int reset) { return gsr::debug_dup_times(out8, reset); }
#endif

}  // extern "C"
