// api.hip -- the render path of the C ABI of include/gsr.h: argument checks, arena carving, kernel sequencing.  The host state behind it
// is host.hpp / host.hip, the process-wide switches are switches.hpp, and the entries only tests and measurements call are inspect.hip.
//
// Host orchestration corresponding to reference CR/rasterizer_impl.cu:198-336 (Rasterizer::forward) and
// :340-434 (Rasterizer::backward), re-planned for this library's data flow.  One submission covers a BATCH of V camera
// views of one cloud (V = 1 for the reference's per-view API); every launch below has the view as a grid dimension.
//
//   forward   preprocess (+ clears the frame's bookkeeping)      1 launch
//             depth sort of the P Gaussians                       4 passes x 3 launches, u32 key / u32 id
//             pair emission in depth order with its own prefix sum  1 launch     -> num_rendered, ON THE DEVICE
//             tile sort                                           ceil(bit/8) passes x 3 launches, u16|u32 tile / u32 id
//             tile ranges (search), tile order by work estimate   2 launches
//             render                                              1 launch
//   backward  work items, render backward, per-Gaussian backward  3 launches
//
// No host round trip inside a frame: where the reference blocks on a device->host copy of num_rendered to size its
// binning buffer (CR/rasterizer_impl.cu:279-285), the binning arena here is carved by CAPACITY (what the caller
// allocated; the Python layer sizes it from the previous frames of the same configuration), every kernel behind the pair
// emission takes its element count from device memory, and the 16-byte counter copy is enqueued right after the emission
// but only waited for once the WHOLE frame has been enqueued.  If a view's count exceeds the capacity the call returns
// GSR_RETRY with the true counts and the caller repeats the binning half with a larger arena (resume = 1).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "adam_step.hpp"
#include "common.hpp"
#include "density_control.hpp"
#include "host.hpp"
#include "image_loss.hpp"
#include "switches.hpp"

namespace gsr {

// pairs in the lists of the calling thread's last forward, per view (<= num_rendered: footprint clipping); gsr_last_list_pairs
static thread_local std::vector<int64_t> t_list_pairs;

// device->host read-backs the library has issued since it was loaded (one per forward call: the per-view counters)
static std::atomic<long long> g_d2h_count{0};

static int check_params(const gsr_params* p, int V = 1)
{
    if (!p) return fail(GSR_ERR_INVALID, "[gsr] params is NULL");
    if (p->P < 0 || p->W <= 0 || p->H <= 0) return fail(GSR_ERR_INVALID, "[gsr] bad sizes P=%d W=%d H=%d", p->P, p->W, p->H);
    if (V < 1 || V > MAX_VIEWS) return fail(GSR_ERR_INVALID, "[gsr] view count %d outside 1..%d", V, MAX_VIEWS);
    if (p->P == 0) return GSR_OK;
    if (!p->means3D || !p->opacities || !p->bg || !p->viewmatrix || !p->projmatrix || !p->campos)
        return fail(GSR_ERR_INVALID, "[gsr] a required input pointer is NULL");
    if ((p->shs == nullptr) == (p->colors_precomp == nullptr))
        return fail(GSR_ERR_INVALID, "Please provide excatly one of either SHs or precomputed colors!");
    if (((p->scales == nullptr || p->rotations == nullptr) && p->cov3D_precomp == nullptr) ||
        ((p->scales != nullptr || p->rotations != nullptr) && p->cov3D_precomp != nullptr))
        return fail(GSR_ERR_INVALID, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    if (p->shs) {
        if (p->D < 0 || p->D > 3) return fail(GSR_ERR_INVALID, "[gsr] SH degree %d outside 0..3", p->D);
        if ((p->D + 1) * (p->D + 1) > p->M) return fail(GSR_ERR_INVALID, "[gsr] SH degree %d needs %d coefficients, M=%d", p->D, (p->D + 1) * (p->D + 1), p->M);
    }
    const int64_t gx = (p->W + TILE_X - 1) / TILE_X, gy = (p->H + TILE_Y - 1) / TILE_Y;
    if (gx > 65535 || gy > 65535) return fail(GSR_ERR_INVALID, "[gsr] image too large for 16-bit tile coordinates");
    // backward work items carry the tile in BWD_TILE_BITS bits, and the render grids hold 4 workgroups per tile and view
    if (gx * gy > (1ll << BWD_TILE_BITS) || (gx * gy / 8 + 1) * 64 * V > 0x7FFFFFFFll)   // (64: the half-quadrant forward's grid)
        return fail(GSR_ERR_INVALID, "[gsr] %lld tiles x %d views: too many for one launch", (long long)(gx * gy), V);
    return GSR_OK;
}

// Carve the caller's three allocations into V per-view arenas.  binning may be NULL (count-only forward).  with_grad: the
// V gradient-record blocks that follow the V geometry arenas are part of the geometry allocation (need_backward calls).
// the geometry half of make_batch, all gsr_backward_cameras needs: the V geometry arenas and the gradient records behind them
static int make_geom_batch(const gsr_params* p, int V, void* geom, size_t geom_bytes, bool with_grad, Batch& B)
{
    B.V = V;
    const size_t G = geom_view(nullptr, p->P).bytes;
    const size_t GR = with_grad ? grad_rec_bytes(p->P) : 0;
    if (!geom || geom_bytes < (size_t)V * (G + GR) + 256)
        return fail(GSR_ERR_CAPACITY, "[gsr] geom arena too small (%zu < %zu%s)", geom_bytes, (size_t)V * (G + GR) + 256,
                    with_grad ? ", need_backward" : "");
    B.g = geom_view(align256(geom), p->P);
    B.g_stride = G;
    B.grad_rec = with_grad ? reinterpret_cast<float*>(reinterpret_cast<char*>(align256(geom)) + (size_t)V * G) : nullptr;
    B.gr_stride = GR;
    return GSR_OK;
}

static int make_batch(const gsr_params* p, int V, void* geom, size_t geom_bytes, void* image, size_t image_bytes, void* binning,
                      size_t binning_bytes, bool with_grad, Batch& B)
{
    const size_t I = image_view(nullptr, p->W, p->H).bytes;
    if (int e = make_geom_batch(p, V, geom, geom_bytes, with_grad, B)) return e;
    if (!image || image_bytes < (size_t)V * I + 256)
        return fail(GSR_ERR_CAPACITY, "[gsr] image arena too small (%zu < %zu)", image_bytes, (size_t)V * I + 256);
    B.iv = image_view(align256(image), p->W, p->H);
    B.iv_stride = I;
    if (binning) {
        if (binning_bytes < 256 + 256 * (size_t)V) return fail(GSR_ERR_CAPACITY, "[gsr] binning arena too small");
        const size_t per_view = ((binning_bytes - 256) / (size_t)V) / 256 * 256;
        const int64_t cap = bin_capacity_from_bytes(per_view);
        if (cap < 1) return fail(GSR_ERR_CAPACITY, "[gsr] binning arena too small (%zu bytes for %d views)", binning_bytes, V);
        B.b = bin_view(align256(binning), cap > 0xFFFFFFFFll ? 0xFFFFFFFFll : cap);
        B.b_stride = per_view;
    } else {
        B.b = bin_view(nullptr, 1);
        B.b.cap = 0;
        B.b_stride = 0;
    }
    return GSR_OK;
}

// per-view bytes of the extra-channel state for a binning arena of capacity cap
static size_t xstate_view_bytes(int W, int H, int64_t cap, int nx) { return align_up(xstate_view(nullptr, W, H, cap, nx).bytes, 256); }

static int memset_views(hipStream_t s, void* base, size_t stride, size_t bytes, int V)
{
    if (bytes == 0) return GSR_OK;
    hipError_t e = V == 1 ? hipMemsetAsync(base, 0, bytes, s) : hipMemset2DAsync(base, stride, 0, bytes, (size_t)V, s);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "[gsr] memset failed: %s", hipGetErrorString(e));
}

// one block to zero in stream order
static int zero_async(hipStream_t s, void* dst, size_t bytes)
{
    if (hipMemsetAsync(dst, 0, bytes, s) == hipSuccess) return GSR_OK;
    return fail(GSR_ERR_HIP, "[gsr] memset failed: %s", hipGetErrorString(hipGetLastError()));
}

// The whole forward for a batch.  mode 0: everything; 1 (resume): from the pair emission on, after a GSR_RETRY or a
// count-only call; 2 (count only): geometry + pair counting, no binning arena.
static int forward_impl(const gsr_params* p, int V, void* geom, size_t geom_bytes, void* image, size_t image_bytes, void* binning,
                        size_t binning_bytes, int* radii, float* out_color, int64_t* num_rendered, int mode, hipStream_t stream,
                        const ExtraChannels* X = nullptr)
{
    if (int e = check_params(p, V)) return e;
    if (!num_rendered) return fail(GSR_ERR_INVALID, "[gsr] num_rendered is NULL");
    for (int v = 0; v < V; v++) num_rendered[v] = 0;
    if (p->P == 0) return GSR_OK;  // reference rasterize_points.cu:81: nothing runs, image stays zero
    if (mode != 1 && !radii) return fail(GSR_ERR_INVALID, "[gsr] radii is NULL");
    if (mode != 2 && !out_color) return fail(GSR_ERR_INVALID, "[gsr] out_color is NULL");
    if (mode != 2 && !binning) return fail(GSR_ERR_INVALID, "[gsr] binning arena is NULL");
    Batch B;
    if (int e = make_batch(p, V, geom, geom_bytes, image, image_bytes, mode == 2 ? nullptr : binning, binning_bytes,
                           p->need_backward != 0, B))
        return e;
    // gsr_forward_batch_channels_train hands its extra-state block over as (state.accum = base, state.bytes = size): carved here
    // for this binning arena's capacity (a resumed call carves it anew for the larger arena)
    ExtraChannels Xs;
    const void* xraw = X != nullptr ? (const void*)X->state.accum : nullptr;
    if (X != nullptr && X->state.accum != nullptr) {
        Xs = *X;
        const size_t need = (size_t)V * xstate_view_bytes(p->W, p->H, B.b.cap, X->nx) + 256;
        if (X->state.bytes < need)
            return fail(GSR_ERR_CAPACITY, "[gsr] extra-state block too small (%zu < %zu: V * gsr_extra_state_bytes(W, H, n, nx) for a binning "
                        "arena of V * gsr_binning_bytes(n))", X->state.bytes, need);
        Xs.state = xstate_view(align256(const_cast<float*>(X->state.accum)), p->W, p->H, B.b.cap, X->nx);
        Xs.state_stride = xstate_view_bytes(p->W, p->H, B.b.cap, X->nx);
        if (!p->need_backward) Xs.state = XStateView{nullptr, nullptr, 0};
        X = &Xs;
    }
    const bool fast = forward_fast_math(p->need_backward != 0, X != nullptr && X->nx > 0);
    {
        FrameRecord r(X ? 1 : 0, p, V);
        r.fwd_need_backward = r.need_backward;
        r.math = fast ? 1 : 0;
        if (X) {
            r.nx = X->nx;
            r.layout = X->values_hi ? 2 : X->view_stride ? 1 : 0;
            if (X->state.accum) { r.xstate = xraw; r.xstate_bytes = X->state.bytes; }
        }
        note_frame(geom, r);
    }
    HostLanding* landp = nullptr;
    if (int e = landing(&landp)) return e;
    HostLanding& t_land = *landp;
    const Launch L{stream, p->debug};
    const int T = tile_count(p);
    const int gridx = (p->W + TILE_X - 1) / TILE_X;
    const bool key16 = tile_keys16(T);
    // the emission kernel leaves the counters of every view in mapped host memory (nothing else stores there); cleared before that
    // kernel is enqueued
    memset(t_land.pinned, 0, (size_t)V * 4 * sizeof(uint64_t));

    if (mode == 1) {
        // the first attempt consumed the frame's bookkeeping: clear it again (k_preprocess did it the first time)
        if (int e = memset_views(L.stream, B.g.zero_begin, B.g_stride, B.g.zero_bytes, V)) return e;
        if (int e = memset_views(L.stream, B.iv.zero_begin, B.iv_stride, B.iv.zero_bytes, V)) return e;
    } else {
        if (p->prefiltered)   // the trap word is only looked at for prefiltered calls
            if (int e = memset_views(L.stream, B.g.counters, B.g_stride, 8 * sizeof(uint64_t), V)) return e;
        {
            ProfScope ps("preprocess", L.stream);
            if (int e = launch_preprocess(L, *p, B, radii)) return e;
        }
        {
            ProfScope ps("depth_sort", L.stream);
            SortJob job{{B.g.dkey[0], B.g.dkey[1]}, {B.g.dval[0], B.g.dval[1]}, B.g.hist, B.g.totals, B.g_stride, nullptr, 0, p->P, V};
            job.blk_minmax = B.g.blk_minmax;
            job.sortctl = B.g.sortctl;
            // half-size sort blocks while whole-size ones would leave the chip short of workgroups
            job.small_blocks = div_up(p->P, RS_TILE) * V < 4096;
            int res = 0;
            if (int e = launch_radix_sort_pairs(L, job, /*iota_vals=*/true, 32, &res)) return e;
            // up to 4 passes (B.g.sortctl says how many did something): the ids in depth order are in dval[passes & 1]
        }
    }
    // the event behind the emission kernel is waited for only after the rest of the frame has been enqueued.
    // Once the emission is in the stream it WILL store into the landing zone, whatever happens to the launches behind it: an
    // early return must not leave it pending (the next call of this thread clears the zone from the host and would race
    // with those late stores), so every error path below drains the stream first.
    const auto rest = [&]() -> int {
        {
            ProfScope ps("duplicate", L.stream);
            if (int e = launch_duplicate(L, p->P, B, gridx, key16, t_land.mapped)) return e;
        }
        {
            g_d2h_count++;
            const hipError_t e = hipEventRecord(t_land.ev, L.stream);
            if (e != hipSuccess) return fail(GSR_ERR_HIP, "[gsr] num_rendered read-back: %s", hipGetErrorString(e));
        }
        if (mode != 2) {
            const int res = sorted_buffer(T);
            {
                ProfScope ps("tile_sort", L.stream);
                SortJob job{{B.b.key[0], B.b.key[1]}, {B.b.val[0], B.b.val[1]}, B.b.hist, B.b.totals, B.b_stride,
                            B.g.counters + CNT_NUM_RENDERED, B.g_stride, B.b.cap, V};
                int r2 = 0;
                if (int e = launch_radix_sort_pairs(L, job, false, tile_bits(T), &r2, key16)) return e;
            }
            {
                ProfScope ps("tile_ranges", L.stream);
                // (one launch of one workgroup per view doing both was measured: 47 us instead of 7 + 11 for a single view --
                // 8 160 binary searches are ~100 000 scattered line requests, and ONE CU's address unit passes about one line
                // per cycle; the search wants its 32 workgroups.  profiles/r06_lookback_sort.txt)
                if (int e = launch_tile_ranges(L, B, B.b.key[res], T, key16)) return e;
                if (int e = launch_tile_order(L, B, T)) return e;
            }
            {
                ProfScope ps("render_forward", L.stream);
                if (int e = launch_render_forward(L, *p, B, B.b.val[res], out_color, p->need_backward != 0, fast, X)) return e;
            }
        }
        return GSR_OK;
    };
    if (int e = rest()) {
        (void)hipStreamSynchronize(L.stream);   // (keeps g_err: the failure being reported)
        return e;
    }
    if (hipEventSynchronize(t_land.ev) != hipSuccess)
        return fail(GSR_ERR_HIP, "[gsr] num_rendered read-back failed: %s", hipGetErrorString(hipGetLastError()));
    bool retry = false;
    t_list_pairs.assign((size_t)V, 0);
    for (int v = 0; v < V; v++) {
        // R: pairs of the reference's tile rectangles (what the reference calls num_rendered); L: pairs in this library's
        // lists (fewer when the rectangles are clipped to the splats' footprints) -- the arena has to hold L
        const uint64_t R = t_land.pinned[4 * v + LAND_NUM_REFERENCE], Lp = t_land.pinned[4 * v + CNT_NUM_RENDERED];
        if (t_land.pinned[4 * v + CNT_STALL])
            return fail(GSR_ERR_HIP, "[gsr] pair emission: a workgroup's pair count never arrived (view %d)", v);
        if (p->prefiltered && t_land.pinned[4 * v + CNT_TRAP])
            return fail(GSR_ERR_TRAP, "Point is filtered although prefiltered is set. This shouldn't happen!");
        // the reference keeps num_rendered in an int (CR/rasterizer_impl.cu:280); beyond that its arena sizes wrap
        if (R > 0x7FFFFFFFull)
            return fail(GSR_ERR_CAPACITY, "[gsr] num_rendered = %llu tile pairs does not fit the reference's int (scales too large?)",
                        (unsigned long long)R);
        num_rendered[v] = (int64_t)R;
        t_list_pairs[(size_t)v] = (int64_t)Lp;
        if (mode != 2 && (int64_t)Lp > B.b.cap) retry = true;
    }
    // the lists' extent joins the arena's record (host data of the one read-back above: gsr_backward_batch_det sizes by it)
    update_frame(geom, [](FrameRecord& r) { r.list_pairs = *std::max_element(t_list_pairs.begin(), t_list_pairs.end()); });
    if (retry) {
        fail(GSR_RETRY, "[gsr] binning arena holds %lld pairs per view, the frame needs more (num_rendered is enough; gsr_last_list_pairs is exact): repeat with resume = 1",
             (long long)B.b.cap);
        return GSR_RETRY;
    }
    return GSR_OK;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_geom_bytes(int P) { return geom_view(nullptr, P).bytes + grad_rec_bytes(P) + 256; }
size_t gsr_geom_bytes_inference(int P) { return geom_view(nullptr, P).bytes + 256; }
size_t gsr_image_bytes(int W, int H) { return image_view(nullptr, W, H).bytes + 256; }
size_t gsr_binning_bytes(int64_t R) { return bin_view(nullptr, R).bytes + 256; }

int gsr_forward_batch(const gsr_params* p, int V, void* geom, size_t geom_bytes, void* image, size_t image_bytes, void* binning,
                      size_t binning_bytes, int* radii, float* out_color, int64_t* num_rendered, int resume, gsr_stream_t stream)
{
    return forward_impl(p, V, geom, geom_bytes, image, image_bytes, binning, binning_bytes, radii, out_color, num_rendered,
                        resume ? 1 : 0, (hipStream_t)stream);
}

static int extra_channels(const gsr_params* p, int nx, int extra_per_view, const float* extra, const float* extra_view_scale,
                          const float* bg_extra, float* out_extra, ExtraChannels& X)
{
    if (!p) return fail(GSR_ERR_INVALID, "[gsr] params is NULL");
    if (nx != 4 && nx != 8) return fail(GSR_ERR_INVALID, "[gsr] extra channels come in 4 or 8 (got %d): pad with zeros", nx);
    if (!extra || !bg_extra || !out_extra) return fail(GSR_ERR_INVALID, "[gsr] an extra-channel pointer is NULL");
    if (extra_per_view < 0 || extra_per_view > 2 || (extra_per_view == 2 && nx != 8))
        return fail(GSR_ERR_INVALID, "[gsr] extra_per_view is 0, 1 or (with 8 channels) 2");
    X = ExtraChannels{nx, extra, extra_view_scale, bg_extra, out_extra, extra_per_view == 1 ? (size_t)p->P * (size_t)nx : (size_t)0};
    if (extra_per_view == 2) {   // [P][4] shared by the views, then [V][P][4]
        X.values_hi = extra + (size_t)p->P * 4;
        X.hi_view_stride = (size_t)p->P * 4;
    }
    return GSR_OK;
}

int gsr_forward_batch_channels(const gsr_params* p, int V, void* geom, size_t geom_bytes, void* image, size_t image_bytes,
                               void* binning, size_t binning_bytes, int* radii, float* out_color, int64_t* num_rendered, int resume,
                               int nx, int extra_per_view, const float* extra, const float* extra_view_scale, const float* bg_extra,
                               float* out_extra, gsr_stream_t stream)
{
    ExtraChannels X;
    if (int e = extra_channels(p, nx, extra_per_view, extra, extra_view_scale, bg_extra, out_extra, X)) return e;
    return forward_impl(p, V, geom, geom_bytes, image, image_bytes, binning, binning_bytes, radii, out_color, num_rendered,
                        resume ? 1 : 0, (hipStream_t)stream, &X);
}

size_t gsr_extra_state_bytes(int W, int H, int64_t num_rendered, int nx)
{
    if (W <= 0 || H <= 0 || (nx != 4 && nx != 8)) return 0;
    // the capacity a binning arena of V * gsr_binning_bytes(num_rendered) bytes is carved for (make_batch)
    return xstate_view_bytes(W, H, bin_capacity_from_bytes(bin_view(nullptr, num_rendered).bytes), nx);
}

int gsr_forward_batch_channels_train(const gsr_params* p, int V, void* geom, size_t geom_bytes, void* image, size_t image_bytes,
                                     void* binning, size_t binning_bytes, int* radii, float* out_color, int64_t* num_rendered,
                                     int resume, int nx, int extra_per_view, const float* extra, const float* extra_view_scale,
                                     const float* bg_extra, float* out_extra, void* extra_state, size_t extra_state_bytes,
                                     gsr_stream_t stream)
{
    ExtraChannels X;
    if (int e = extra_channels(p, nx, extra_per_view, extra, extra_view_scale, bg_extra, out_extra, X)) return e;
    if (!extra_state) return fail(GSR_ERR_INVALID, "[gsr] extra_state is NULL");
    X.state = XStateView{reinterpret_cast<float*>(extra_state), nullptr, extra_state_bytes};
    return forward_impl(p, V, geom, geom_bytes, image, image_bytes, binning, binning_bytes, radii, out_color, num_rendered,
                        resume ? 1 : 0, (hipStream_t)stream, &X);
}

int gsr_forward_stage1(const gsr_params* p, void* geom, size_t geom_bytes, void* image, size_t image_bytes, int* radii,
                       int64_t* num_rendered_out, gsr_stream_t stream)
{
    if (!num_rendered_out) return fail(GSR_ERR_INVALID, "[gsr] num_rendered_out is NULL");
    return forward_impl(p, 1, geom, geom_bytes, image, image_bytes, nullptr, 0, radii, nullptr, num_rendered_out, 2, (hipStream_t)stream);
}

int gsr_forward_stage2(const gsr_params* p, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes, void* image,
                       size_t image_bytes, int64_t R, float* out_color, gsr_stream_t stream)
{
    if (R < 0 || R > 0x7FFFFFFFll) return fail(GSR_ERR_INVALID, "[gsr] num_rendered out of range");
    if (p && p->P > 0 && (!binning || binning_bytes < gsr_binning_bytes(R)))
        return fail(GSR_ERR_CAPACITY, "[gsr] binning arena too small (%zu < %zu)", binning_bytes, gsr_binning_bytes(R));
    int64_t got = 0;
    const int rc = forward_impl(p, 1, geom, geom_bytes, image, image_bytes, binning, binning_bytes, nullptr, out_color, &got, 1,
                                (hipStream_t)stream);
    if (rc == GSR_OK && p && p->P > 0 && got != R) return fail(GSR_ERR_INVALID, "[gsr] stage 2 found %lld pairs, stage 1 reported %lld", (long long)got, (long long)R);
    return rc;
}

// Colour-only re-render on the geometry / lists of a finished forward (same P, views, image size).
int gsr_forward_recolor(const gsr_params* p, int V, int colors_per_view, void* geom, size_t geom_bytes, const void* binning,
                        size_t binning_bytes, void* image, size_t image_bytes, float* out_color, gsr_stream_t stream)
{
    if (!p) return fail(GSR_ERR_INVALID, "[gsr] params is NULL");
    if (V < 1 || V > MAX_VIEWS) return fail(GSR_ERR_INVALID, "[gsr] view count %d outside 1..%d", V, MAX_VIEWS);
    if (p->P <= 0) return GSR_OK;
    if ((p->shs == nullptr) == (p->colors_precomp == nullptr))
        return fail(GSR_ERR_INVALID, "Please provide excatly one of either SHs or precomputed colors!");
    if (p->shs && (!p->means3D || !p->campos || p->D < 0 || p->D > 3 || (p->D + 1) * (p->D + 1) > p->M))
        return fail(GSR_ERR_INVALID, "[gsr] recolor: bad SH arguments");
    if (!out_color || !p->bg || !binning) return fail(GSR_ERR_INVALID, "[gsr] recolor: NULL pointer");
    Batch B;
    if (int e = make_batch(p, V, geom, geom_bytes, image, image_bytes, const_cast<void*>(binning), binning_bytes, false, B)) return e;
    const bool fast = forward_fast_math(p->need_backward != 0, false);
    {
        // a need_backward recolor rewrites the colour saves only: the gradient records and the SH clamp mask of the other Gaussians
        // exist (and were cleared) only if the forward under it had need_backward too
        FrameRecord prev, r(2, p, V);
        r.math = fast ? 1 : 0;
        if (find_frame(geom, prev)) {   // (no record: both stay -1, unknown)
            r.fwd_need_backward = prev.fwd_need_backward;
            r.list_pairs = prev.list_pairs;
        }
        note_frame(geom, r);
    }
    const Launch L{(hipStream_t)stream, p->debug};
    const int res = sorted_buffer(tile_count(p));
    {
        ProfScope ps("recolor", L.stream);
        if (int e = launch_recolor(L, *p, B, (colors_per_view && p->colors_precomp) ? (size_t)p->P * 3 : 0)) return e;
        // the render accumulates the consumed-entry counts from zero
        if (int e = memset_views(L.stream, B.iv.tile_need, B.iv_stride, (size_t)tile_count(p) * sizeof(uint32_t), V)) return e;
    }
    {
        ProfScope ps("render_forward", L.stream);
        // need_backward: the slice-boundary state and the accumulated colour are rewritten for the new colours (and k_recolor
        // refreshed the SH clamp mask), so a backward afterwards differentiates this render
        if (int e = launch_render_forward(L, *p, B, B.b.val[res], out_color, p->need_backward != 0, fast)) return e;
    }
    return GSR_OK;
}

// total bytes of a deterministic backward's scratch block for lists of up to `pairs` pairs per view (nx = 0: the colour backward)
static size_t det_bytes(int V, int P, int W, int H, int64_t pairs, int nx, int extra_per_view)
{
    if (V < 1 || W <= 0 || H <= 0) return 0;
    const int T = ((W + TILE_X - 1) / TILE_X) * ((H + TILE_Y - 1) / TILE_Y);
    return det_scratch(nullptr, V, P, T, pairs, nx, extra_per_view).bytes;
}

// (P does not enter: the sort's key bits follow P, its work space does not)
size_t gsr_backward_det_bytes(int V, int P, int W, int H, int64_t pairs) { return det_bytes(V, P, W, H, pairs, 0, 0); }

size_t gsr_backward_det_channels_bytes(int V, int P, int W, int H, int64_t pairs, int nx, int extra_per_view)
{
    if ((nx != 4 && nx != 8) || extra_per_view < 0 || extra_per_view > 2 || (extra_per_view == 2 && nx != 8)) return 0;
    return det_bytes(V, P, W, H, pairs, nx, extra_per_view);
}

// ---- the backward: one sequence behind gsr_backward, gsr_backward_batch, gsr_backward_batch_det, gsr_backward_batch_channels and
// gsr_backward_batch_channels_det ----
struct BwdGrads {   // dL/d image in, the eight gradient outputs (include/gsr.h)
    const float* dL_dpix;
    float *dL_dmean2D, *dL_dopacity, *dL_dcolor, *dL_dmean3D, *dL_dcov3D, *dL_dsh, *dL_dscale, *dL_drot;
};
struct BwdDet { void* scratch; size_t bytes; };   // optional part: the deterministic backward's scratch block
struct BwdExtra {   // optional part: the extra channels (X.state is carved by backward_impl), their gradients and state block
    ExtraChannels X;
    ExtraGrads XG;
    int layout;     // extra_per_view
    const void* state;
    size_t state_bytes;
};

static int check_bwd_pointers(const gsr_params* p, const int* radii, const void* binning, const BwdGrads& G)
{
    if (!radii || !G.dL_dpix || !G.dL_dmean2D || !G.dL_dopacity || !G.dL_dcolor || !G.dL_dmean3D || !G.dL_dcov3D)
        return fail(GSR_ERR_INVALID, "[gsr] a required backward pointer is NULL");
    if (p->shs && !G.dL_dsh) return fail(GSR_ERR_INVALID, "[gsr] dL_dsh is NULL");
    if (p->scales && (!G.dL_dscale || !G.dL_drot)) return fail(GSR_ERR_INVALID, "[gsr] dL_dscale/dL_drot is NULL");
    if (p->scales && ((uintptr_t)G.dL_drot & 15u)) return fail(GSR_ERR_INVALID, "[gsr] dL_drot must be 16-byte aligned (it is written one float4 per Gaussian)");
    if (!binning) return fail(GSR_ERR_INVALID, "[gsr] binning arena is NULL");
    return GSR_OK;
}

// The forward or recolor a backward differentiates has to have saved what it reads, for the same views and sizes.
// Colour backward (x == NULL): frame_gate, and between its first and its last question a rule of this entry's own (a need_backward
// recolor needs the arenas of a need_backward forward).  Channels backward: the record has to be that of a channels forward with
// need_backward = 1 into this extra-state block, with the same channels, layout and sizes.  list_pairs: the record's (-1: none).
// math: the arithmetic the saves were written in, from the record; without one, the training switch in force (the caller then has
// to keep it where the forward had it).
static int check_bwd_frame(const void* geom, const gsr_params* p, int V, const BwdExtra* x, int64_t* list_pairs, int* math)
{
    FrameRecord r;
    *list_pairs = -1;
    *math = x ? 0 : train_math(-1);
    if (!x) {
        bool known = false;
        const int e = frame_gate("backward", geom, p, V, GATE_SAVES, " and saved nothing for it", &r, &known);
        if (!known) return GSR_OK;
        *list_pairs = r.list_pairs;
        *math = r.math;
        if (r.need_backward && r.fwd_need_backward == 0)   // (comes before the gate's answer about the sizes)
            return fail(GSR_ERR_INVALID, "[gsr] backward: the recolor's forward on this geometry arena had need_backward = 0 (a "
                        "need_backward recolor needs the arenas of a need_backward forward)");
        return e;
    }
    if (!find_frame(geom, r))
        return fail(GSR_ERR_INVALID, "[gsr] backward_channels: no forward on this geometry arena (run gsr_forward_batch_channels_train first)");
    *list_pairs = r.list_pairs;
    *math = r.math;
    const bool same = r.V == V && r.P == p->P && r.W == p->W && r.H == p->H;
    if (r.kind == 2)
        return fail(GSR_ERR_INVALID, "[gsr] backward_channels after gsr_forward_recolor is not supported: the recolor replaced the saves "
                    "of the channels forward (run gsr_forward_batch_channels_train again)");
    if (r.kind != 1 || !r.need_backward || r.xstate == nullptr)
        return fail(GSR_ERR_INVALID, "[gsr] backward_channels: the forward on this arena saved no extra channels (it needs "
                    "gsr_forward_batch_channels_train with need_backward = 1)");
    if (r.nx != x->X.nx || r.layout != x->layout)
        return fail(GSR_ERR_INVALID, "[gsr] backward_channels: nx = %d, extra_per_view = %d, but the forward had nx = %d, extra_per_view = %d",
                    x->X.nx, x->layout, r.nx, r.layout);
    if (!same) return fail(GSR_ERR_INVALID, "[gsr] backward_channels: views / sizes differ from the forward's");
    if (r.xstate != x->state || x->state_bytes < r.xstate_bytes)
        return fail(GSR_ERR_INVALID, "[gsr] backward_channels: extra_state is not the block the forward saved into");
    return GSR_OK;
}

// det / x: the two optional parts; both = the deterministic channels backward (the scratch block then also holds the extras' slots
// and the staging of the rows the views share).
static int backward_impl(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                         size_t binning_bytes, const void* image, size_t image_bytes, const BwdGrads& G, const BwdDet* det, BwdExtra* x,
                         gsr_stream_t stream)
{
    if (int e = check_params(p, V)) return e;
    if (p->P == 0) return GSR_OK;
    // which fault a call with several reports is part of each entry's contract: the colour entries look at the pointers first, the
    // channels entry at the arena's record
    int64_t list_pairs = -1;
    if (!x)
        if (int e = check_bwd_pointers(p, radii, binning, G)) return e;
    int math = 0;
    if (int e = check_bwd_frame(geom, p, V, x, &list_pairs, &math)) return e;
    if (x)
        if (int e = check_bwd_pointers(p, radii, binning, G)) return e;
    Batch B;
    if (int e = make_batch(p, V, const_cast<void*>(geom), geom_bytes, const_cast<void*>(image), image_bytes,
                           const_cast<void*>(binning), binning_bytes, true, B))
        return e;
    const Launch L{(hipStream_t)stream, p->debug};
    const int T = tile_count(p), res = sorted_buffer(T);
    if (x) {
        const int nx = x->X.nx;
        x->X.state = xstate_view(align256(const_cast<void*>(x->state)), p->W, p->H, B.b.cap, nx);
        x->X.state_stride = xstate_view_bytes(p->W, p->H, B.b.cap, nx);
        if (x->state_bytes < (size_t)V * x->X.state_stride + 256)
            return fail(GSR_ERR_CAPACITY, "[gsr] extra-state block too small for this binning arena");
    }
    // deterministic: one slot per (consumed list entry, quadrant) in the caller's scratch block.  The block has to hold the
    // forward's lists: their largest per-view pair count from the arena's record, or -- no record -- the binning arena's capacity
    DetScratch S{};
    if (det) {
        int64_t n = list_pairs >= 0 ? list_pairs : B.b.cap;
        if (n > B.b.cap) n = B.b.cap;
        if (n < 1) n = 1;
        S = det_scratch(align256(det->scratch), V, p->P, T, n, x ? x->X.nx : 0, x ? x->layout : 0);
        if (!det->scratch || det->bytes < S.bytes)
            return x ? fail(GSR_ERR_CAPACITY, "[gsr] backward_channels_det: scratch block too small (%zu < %zu = "
                            "gsr_backward_det_channels_bytes(%d, %d, %d, %d, %lld, %d, %d): the forward's lists hold up to %lld pairs per "
                            "view)", det->bytes, S.bytes, V, p->P, p->W, p->H, (long long)n, x->X.nx, x->layout, (long long)n)
                     : fail(GSR_ERR_CAPACITY, "[gsr] backward_det: scratch block too small (%zu < %zu = gsr_backward_det_bytes(%d, %d, %d, "
                            "%d, %lld): the forward's lists hold up to %lld pairs per view)", det->bytes, S.bytes, V, p->P, p->W, p->H,
                            (long long)n, (long long)n);
    }
    {
        ProfScope ps("bwd_items", L.stream);
        // dL/d extra values are accumulated with atomics, views that share an array into the same rows: clear the output first
        // (deterministic: the ordered reduction writes the rows of the Gaussians it reaches with plain stores; the others stay zero,
        // in the caller's per-view rows and in the staging of the shared ones)
        const size_t n_out = !x ? 0 : (size_t)p->P * (x->layout == 0 ? x->X.nx : x->layout == 1 ? V * x->X.nx : (1 + V) * 4);
        if (x)
            if (int e = zero_async(L.stream, x->XG.grad, n_out * sizeof(float))) return e;
        if (S.stage)
            if (int e = zero_async(L.stream, S.stage, (size_t)V * S.n_stage * sizeof(float))) return e;
        if (int e = launch_bwd_items(L, B, T, p->P)) return e;
    }
    int dres = 0;
    if (det) {
        {
            ProfScope ps("det_prepare", L.stream);
            if (int e = launch_det_prepare(L, B, S, B.b.val[res], T)) return e;
        }
        {
            ProfScope ps("det_sort", L.stream);
            if (int e = launch_det_sort(L, B, S, p->P, &dres)) return e;
        }
    }
    {
        ProfScope ps("render_backward", L.stream);
        const RenderBwdDet d{S.d.part, S.d.flags, S.d.slot_base, S.stride, (uint32_t)S.d.cap};
        // (storing channels kernels: the extras' sums go to the scratch block's slots, not to the caller's output)
        const ExtraGrads xg_slots{x ? x->XG.dL_dextra : nullptr, S.xpart, nullptr};
        if (int e = launch_render_backward(L, *p, B, B.b.val[res], G.dL_dpix, x ? &x->X : nullptr, !x ? nullptr : det ? &xg_slots : &x->XG,
                                           det ? &d : nullptr, !x && math == 1))
            return e;
    }
    if (det) {
        ProfScope ps("det_reduce", L.stream);
        if (int e = launch_det_reduce(L, B, S, dres)) return e;
    }
    if (det && x) {
        ProfScope ps("det_reduce_extra", L.stream);
        if (int e = launch_det_reduce_extra(L, B, S, dres, p->P, x->X.nx, x->layout, x->XG)) return e;
    }
    if (S.stage) {
        ProfScope ps("det_viewsum", L.stream);
        if (int e = launch_det_viewsum(L, B, S, x->XG)) return e;
    }
    {
        ProfScope ps("preprocess_backward", L.stream);
        if (int e = launch_preprocess_backward(L, *p, B, radii, G.dL_dmean2D, G.dL_dopacity, G.dL_dcolor, G.dL_dmean3D, G.dL_dcov3D,
                                               G.dL_dsh, G.dL_dscale, G.dL_drot))
            return e;
    }
    // the records now hold this backward's per-view sums: gsr_backward_cameras may follow
    update_frame(geom, [](FrameRecord& r) { r.bwd_done = 1; });
    return GSR_OK;
}

int gsr_backward_batch(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                       size_t binning_bytes, const void* image, size_t image_bytes, const float* dL_dpix, float* dL_dmean2D,
                       float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                       float* dL_drot, gsr_stream_t stream)
{
    const BwdGrads G{dL_dpix, dL_dmean2D, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot};
    return backward_impl(p, V, radii, geom, geom_bytes, binning, binning_bytes, image, image_bytes, G, nullptr, nullptr, stream);
}

int gsr_backward_batch_det(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                           size_t binning_bytes, const void* image, size_t image_bytes, const float* dL_dpix, float* dL_dmean2D,
                           float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                           float* dL_drot, void* det_scratch, size_t det_scratch_bytes, gsr_stream_t stream)
{
    const BwdGrads G{dL_dpix, dL_dmean2D, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot};
    const BwdDet det{det_scratch, det_scratch_bytes};
    return backward_impl(p, V, radii, geom, geom_bytes, binning, binning_bytes, image, image_bytes, G, &det, nullptr, stream);
}

// the two channels entries: det == NULL is the atomic one
static int backward_channels(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                             size_t binning_bytes, const void* image, size_t image_bytes, const BwdGrads& G, int nx, int extra_per_view,
                             const float* extra, const float* extra_view_scale, const float* bg_extra, const void* extra_state,
                             size_t extra_state_bytes, const float* dL_dextra, float* dL_dextra_values, const BwdDet* det,
                             gsr_stream_t stream)
{
    BwdExtra x{{}, {}, extra_per_view, extra_state, extra_state_bytes};
    if (int e = extra_channels(p, nx, extra_per_view, extra, extra_view_scale, bg_extra, dL_dextra_values, x.X)) return e;
    if (!dL_dextra || !extra_state) return fail(GSR_ERR_INVALID, "[gsr] dL_dextra / extra_state is NULL");
    x.XG = ExtraGrads{dL_dextra, dL_dextra_values, extra_per_view == 2 ? dL_dextra_values + (size_t)p->P * 4 : nullptr};
    return backward_impl(p, V, radii, geom, geom_bytes, binning, binning_bytes, image, image_bytes, G, det, &x, stream);
}

int gsr_backward_batch_channels(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                                size_t binning_bytes, const void* image, size_t image_bytes, const float* dL_dpix, float* dL_dmean2D,
                                float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                                float* dL_dscale, float* dL_drot, int nx, int extra_per_view, const float* extra,
                                const float* extra_view_scale, const float* bg_extra, const void* extra_state, size_t extra_state_bytes,
                                const float* dL_dextra, float* dL_dextra_values, gsr_stream_t stream)
{
    const BwdGrads G{dL_dpix, dL_dmean2D, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot};
    return backward_channels(p, V, radii, geom, geom_bytes, binning, binning_bytes, image, image_bytes, G, nx, extra_per_view, extra,
                             extra_view_scale, bg_extra, extra_state, extra_state_bytes, dL_dextra, dL_dextra_values, nullptr, stream);
}

int gsr_backward_batch_channels_det(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                                    size_t binning_bytes, const void* image, size_t image_bytes, const float* dL_dpix, float* dL_dmean2D,
                                    float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                                    float* dL_dscale, float* dL_drot, int nx, int extra_per_view, const float* extra,
                                    const float* extra_view_scale, const float* bg_extra, const void* extra_state,
                                    size_t extra_state_bytes, const float* dL_dextra, float* dL_dextra_values, void* det_scratch,
                                    size_t det_scratch_bytes, gsr_stream_t stream)
{
    const BwdGrads G{dL_dpix, dL_dmean2D, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot};
    const BwdDet det{det_scratch, det_scratch_bytes};
    return backward_channels(p, V, radii, geom, geom_bytes, binning, binning_bytes, image, image_bytes, G, nx, extra_per_view, extra,
                             extra_view_scale, bg_extra, extra_state, extra_state_bytes, dL_dextra, dL_dextra_values, &det, stream);
}

int gsr_backward(const gsr_params* p, const int* radii, int64_t R, const void* geom, size_t geom_bytes, const void* binning,
                 size_t binning_bytes, const void* image, size_t image_bytes, const float* dL_dpix, float* dL_dmean2D,
                 float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                 float* dL_dscale, float* dL_drot, gsr_stream_t stream)
{
    (void)R;   // the lists' extent lives in the arenas; kept for symmetry with the reference's backward(P, D, M, R, ...)
    return gsr_backward_batch(p, 1, radii, geom, geom_bytes, binning, binning_bytes, image, image_bytes, dL_dpix, dL_dmean2D,
                              dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, stream);
}

// ---- camera gradients: a reduction over the gradient records the last backward on the arenas left (camera_bwd.hip) ----
size_t gsr_camera_grad_bytes(int V, int P)
{
    if (V < 1 || V > MAX_VIEWS || P < 0) return 0;
    return align_up(camera_slab_bytes(V, P), 256) + 256;   // (+ 256 for aligning the caller's pointer)
}

int gsr_backward_cameras(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, float* dL_dviewmatrix,
                         float* dL_dprojmatrix, float* dL_dcampos, void* scratch, size_t scratch_bytes, gsr_stream_t stream)
{
    if (int e = check_params(p, V)) return e;
    if (p->P == 0) return GSR_OK;
    if (!radii || !geom || !dL_dviewmatrix || !dL_dprojmatrix || !dL_dcampos || !scratch)
        return fail(GSR_ERR_INVALID, "[gsr] backward_cameras: a required pointer is NULL");
    if (scratch_bytes < gsr_camera_grad_bytes(V, p->P))
        return fail(GSR_ERR_CAPACITY, "[gsr] backward_cameras: scratch block too small (%zu < %zu = gsr_camera_grad_bytes(%d, %d))",
                    scratch_bytes, gsr_camera_grad_bytes(V, p->P), V, p->P);
    if (int e = frame_gate("backward_cameras", geom, p, V, GATE_SAVES | GATE_RECORDS, ": there are no gradient records")) return e;
    Batch B;
    if (int e = make_geom_batch(p, V, const_cast<void*>(geom), geom_bytes, true, B)) return e;
    const Launch L{(hipStream_t)stream, p->debug};
    double* slab = reinterpret_cast<double*>(align256(scratch));
    {
        ProfScope ps("camera_partials", L.stream);
        if (int e = launch_camera_partials(L, *p, B, radii, slab)) return e;
    }
    {
        ProfScope ps("camera_sum", L.stream);
        if (int e = launch_camera_sum(L, V, p->P, p->shs != nullptr, slab, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos)) return e;
    }
    return GSR_OK;
}

// ---- density-control statistics and per-view shares: the other reader of the gradient records (view_stats.hip) ----
int gsr_backward_view_stats(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, int accumulate,
                            float* grad_norm_sum, int* visible_views, int* max_radius, float* dL_dmean2D_views,
                            float* dL_dcolor_views, float* dL_dopacity_views, gsr_stream_t stream)
{
    if (int e = check_params(p, V)) return e;
    if (p->P == 0) return GSR_OK;
    if (!radii || !geom) return fail(GSR_ERR_INVALID, "[gsr] backward_view_stats: a required pointer is NULL");
    if (!grad_norm_sum && !visible_views && !max_radius && !dL_dmean2D_views && !dL_dcolor_views && !dL_dopacity_views)
        return fail(GSR_ERR_INVALID, "[gsr] backward_view_stats: all six outputs are NULL: nothing to write");
    if (((uintptr_t)dL_dmean2D_views & 7u) != 0)
        return fail(GSR_ERR_INVALID, "[gsr] backward_view_stats: dL_dmean2D_views is not 8-byte aligned (its rows leave as 8-B stores)");
    if (int e = frame_gate("backward_view_stats", geom, p, V, GATE_SAVES | GATE_RECORDS, ": there are no gradient records")) return e;
    Batch B;
    if (int e = make_geom_batch(p, V, const_cast<void*>(geom), geom_bytes, true, B)) return e;
    const Launch L{(hipStream_t)stream, p->debug};
    ProfScope ps("view_stats", L.stream);
    return launch_view_stats(L, p->P, B, radii, accumulate, grad_norm_sum, visible_views, max_radius, dL_dmean2D_views,
                             dL_dcolor_views, dL_dopacity_views);
}

// ---- per-Gaussian contribution statistics: a read-only walk of the forward's lists (contrib_stats.hip) ----
int gsr_contrib_stats(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                      size_t binning_bytes, const void* image, size_t image_bytes, const float* pixel_weights, int accumulate,
                      float* weight_sum, float* weight_max, int* pixel_count, int* dominant_count, gsr_stream_t stream)
{
    (void)radii;   // a Gaussian that is invisible in a view is in none of its lists
    if (int e = check_params(p, V)) return e;
    if (p->P == 0) return GSR_OK;
    if (!geom || !binning || !image) return fail(GSR_ERR_INVALID, "[gsr] contrib_stats: a required pointer is NULL");
    if (!weight_sum && !weight_max && !pixel_count && !dominant_count)
        return fail(GSR_ERR_INVALID, "[gsr] contrib_stats: all four outputs are NULL: nothing to write");
    if (int e = frame_gate("contrib_stats", geom, p, V, 0, "")) return e;   // (sizes only: the walk reads what every forward leaves)
    Batch B;
    if (int e = make_batch(p, V, const_cast<void*>(geom), geom_bytes, const_cast<void*>(image), image_bytes,
                           const_cast<void*>(binning), binning_bytes, false, B))
        return e;
    const Launch L{(hipStream_t)stream, p->debug};
    ProfScope ps("contrib_stats", L.stream);
    if (!accumulate) {
        void* const outs[4] = {weight_sum, weight_max, pixel_count, dominant_count};
        for (void* o : outs)
            if (o)
                if (int e = zero_async(L.stream, o, (size_t)p->P * 4)) return e;
    }
    return launch_contrib_stats(L, *p, B, B.b.val[sorted_buffer(tile_count(p))], pixel_weights, weight_sum, weight_max, pixel_count,
                                dominant_count);
}

// ---- the photometric loss and its gradient with respect to the frames (image_loss.hip) ----
// checks 1 and 2 of the two entries, which the size query shares (what == NULL: no message, the query just answers 0)
static int image_loss_sizes(const char* what, int V, int W, int H, int ss)
{
    if (V < 1 || V > MAX_VIEWS) return what ? fail(GSR_ERR_INVALID, "[gsr] %s: view count %d outside 1..%d", what, V, MAX_VIEWS) : GSR_ERR_INVALID;
    // (64-bit steps that cannot wrap: W H < 2^62, then 3 V W H < 2^41, then the rate's square)
    const int64_t lim = 1ll << 31, wh = W >= 1 && H >= 1 ? (int64_t)W * (int64_t)H : lim, s2 = (int64_t)ss * (int64_t)ss;
    const int64_t n = wh < lim ? 3 * (int64_t)V * wh : lim;
    if (n >= lim || s2 >= lim || n * (s2 > 0 ? s2 : 1) >= lim || il_parts(W, H) >= (1ll << 24))
        return what ? fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes W=%d H=%d (both >= 1, 3 V H W ss^2 = 3 x %d x %d x %d x %d^2 below 2^31, at most "
                           "2^24 tiles x channels)", what, W, H, V, H, W, ss) : GSR_ERR_INVALID;
    return GSR_OK;
}

// checks 3 and 4
static int image_loss_rate_lambda(const char* what, int ss, float lambda)
{
    if (ss != 1 && ss != 2)
        return fail(GSR_ERR_INVALID, "[gsr] %s: super-sample rate %d is not supported: rate 1 compares the frames as they are, rate 2 is the "
                    "mean of every 2 x 2 block (the bilinear down-filter at that rate); other rates stay with the caller, who down-filters "
                    "first and passes ss = 1", what, ss);
    if (!(lambda >= 0.f && lambda <= 1.f)) return fail(GSR_ERR_INVALID, "[gsr] %s: lambda_dssim = %g outside 0..1", what, (double)lambda);
    return GSR_OK;
}

size_t gsr_image_loss_state_bytes(int V, int W, int H)
{
    if (image_loss_sizes(nullptr, V, W, H, 1) != GSR_OK) return 0;
    return image_loss_state(nullptr, V, W, H).bytes;
}

int gsr_image_loss_forward(int V, int W, int H, int ss, float lambda_dssim, const float* image, const float* target, float* loss_terms,
                           void* state, size_t state_bytes, gsr_stream_t stream)
{
    const char* who = "image_loss_forward";
    if (int e = image_loss_sizes(who, V, W, H, ss)) return e;
    if (int e = image_loss_rate_lambda(who, ss, lambda_dssim)) return e;
    if (!image || !target || !loss_terms) return fail(GSR_ERR_INVALID, "[gsr] %s: image, target or loss_terms is NULL", who);
    ImageLossState S{nullptr, nullptr, 0};
    if (state) {
        S = image_loss_state(align256(state), V, W, H);
        if (state_bytes < S.bytes)
            return fail(GSR_ERR_CAPACITY, "[gsr] %s: state block too small (%zu < %zu = gsr_image_loss_state_bytes(%d, %d, %d))", who,
                        state_bytes, S.bytes, V, W, H);
    }
    const Launch L{(hipStream_t)stream, 0};
    const ImageLossArgs a{V, W, H, ss, image, target};
    ProfScope ps("image_loss_fwd", L.stream);
    return launch_image_loss_forward(L, a, lambda_dssim, loss_terms, S.partials, S.maps);
}

int gsr_image_loss_backward(int V, int W, int H, int ss, float lambda_dssim, const float* image, const float* target,
                            const float* dL_dloss, const void* state, size_t state_bytes, float* dL_dimage, gsr_stream_t stream)
{
    const char* who = "image_loss_backward";
    if (int e = image_loss_sizes(who, V, W, H, ss)) return e;
    if (int e = image_loss_rate_lambda(who, ss, lambda_dssim)) return e;
    if (!image || !target || !dL_dimage || !state) return fail(GSR_ERR_INVALID, "[gsr] %s: image, target, dL_dimage or state is NULL", who);
    const ImageLossState S = image_loss_state(align256(const_cast<void*>(state)), V, W, H);
    if (state_bytes < S.bytes)
        return fail(GSR_ERR_CAPACITY, "[gsr] %s: state block too small (%zu < %zu = gsr_image_loss_state_bytes(%d, %d, %d))", who,
                    state_bytes, S.bytes, V, W, H);
    const Launch L{(hipStream_t)stream, 0};
    const ImageLossArgs a{V, W, H, ss, image, target};
    ProfScope ps("image_loss_bwd", L.stream);
    return launch_image_loss_backward(L, a, lambda_dssim, dL_dloss, S.maps, dL_dimage);
}

// ---- the optimizer step (adam_step.hip): every refusal precedes the first device call ----
int gsr_visible_from_radii(int V, int P, const int32_t* radii, uint8_t* visible, gsr_stream_t stream)
{
    const char* who = "visible_from_radii";
    if (V < 1 || V > MAX_VIEWS) return fail(GSR_ERR_INVALID, "[gsr] %s: view count %d outside 1..%d", who, V, MAX_VIEWS);
    if (P < 1 || (int64_t)V * (int64_t)P >= (1ll << 31))
        return fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes P=%d (at least 1, V P = %d x %d below 2^31)", who, P, V, P);
    if (!radii || !visible) return fail(GSR_ERR_INVALID, "[gsr] %s: radii or visible is NULL", who);
    const Launch L{(hipStream_t)stream, 0};
    ProfScope ps("visible_from_radii", L.stream);
    return launch_visible_from_radii(L, V, P, radii, visible);
}

int gsr_adam_step(int P, int G, const gsr_adam_group* groups, int64_t t, float beta1, float beta2, float eps, const uint8_t* visible,
                  int zero_grads, gsr_stream_t stream)
{
    const char* who = "adam_step";
    if (G < 1 || G > ADAM_MAX_GROUPS) return fail(GSR_ERR_INVALID, "[gsr] %s: group count %d outside 1..%d", who, G, ADAM_MAX_GROUPS);
    // (the table is read for its sizes before its pointers are judged: a NULL table has no sizes to refuse and falls to the last check)
    if (P < 1) return fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes P=%d (at least 1)", who, P);
    for (int k = 0; groups && k < G; k++)
        if (groups[k].width < 1 || (int64_t)P * (int64_t)groups[k].width >= (1ll << 31))
            return fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes in group %d: width %d (at least 1, P width = %d x %d below 2^31)", who, k,
                        groups[k].width, P, groups[k].width);
    if (t < 1) return fail(GSR_ERR_INVALID, "[gsr] %s: step count t = %lld (the first step is t = 1)", who, (long long)t);
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))
        return fail(GSR_ERR_INVALID, "[gsr] %s: beta1 = %g, beta2 = %g outside [0, 1)", who, (double)beta1, (double)beta2);
    if (!(eps > 0.f) || !std::isfinite(eps)) return fail(GSR_ERR_INVALID, "[gsr] %s: eps = %g is not a positive finite number", who, (double)eps);
    for (int k = 0; groups && k < G; k++)
        if (!(groups[k].lr >= 0.f) || !std::isfinite(groups[k].lr))
            return fail(GSR_ERR_INVALID, "[gsr] %s: learning rate %g of group %d is negative or not finite", who, (double)groups[k].lr, k);
    if (!groups) return fail(GSR_ERR_INVALID, "[gsr] %s: groups is NULL", who);
    for (int k = 0; k < G; k++)
        if (!groups[k].param || !groups[k].grad || !groups[k].exp_avg || !groups[k].exp_avg_sq)
            return fail(GSR_ERR_INVALID, "[gsr] %s: param, grad, exp_avg or exp_avg_sq of group %d is NULL", who, k);

    AdamTable T;
    std::memset(&T, 0, sizeof(T));
    T.G = G;
    T.b1 = beta1;
    T.b2 = beta2;
    T.c1 = 1.0f - beta1;
    T.c2 = 1.0f - beta2;
    T.eps = eps;
    T.rsq2 = (float)(1.0 / std::sqrt(1.0 - std::pow((double)beta2, (double)t)));
    T.zero_grads = zero_grads != 0;
    const double bias1 = 1.0 - std::pow((double)beta1, (double)t);
    int64_t units = 0;
    for (int k = 0; k < G; k++) units += div_up((int64_t)P * groups[k].width, ADAM_BLOCK_ELEMS);
    uint32_t end = 0;
    for (int k = 0; k < G; k++) {
        const gsr_adam_group& s = groups[k];
        AdamGroupDev& d = T.g[k];
        d.param = s.param;
        d.grad = s.grad;
        d.exp_avg = s.exp_avg;
        d.exp_avg_sq = s.exp_avg_sq;
        d.n = (uint32_t)((int64_t)P * s.width);
        d.width = (uint32_t)s.width;
        d.block_end = end += adam_group_blocks(d.n, units);
        d.vec = (((uintptr_t)s.param | (uintptr_t)s.grad | (uintptr_t)s.exp_avg | (uintptr_t)s.exp_avg_sq) & 15u) == 0;
        d.step = (float)((double)s.lr / bias1);
    }
    const Launch L{(hipStream_t)stream, 0};
    ProfScope ps("adam_step", L.stream);
    return launch_adam_step(L, T, visible);
}

// ---- adaptive density control (density_control.hip): every refusal precedes the first device call, in the header's order ----
static bool density_sizes_ok(int P) { return P >= 1 && 2 * (int64_t)P < (1ll << 31); }

// a rule the kernels can take: thresholds and sizes are non-negative finite numbers, min_opacity is a number
static int density_rule_check(const char* who, const gsr_density_rule* r)
{
    if (!r) return GSR_OK;   // a NULL rule has no values to refuse and falls to the pointer check
    if (!(r->grad_threshold >= 0.f) || !std::isfinite(r->grad_threshold) || !(r->dense_size >= 0.f) || !std::isfinite(r->dense_size) ||
        !(r->max_world_size >= 0.f) || !std::isfinite(r->max_world_size) || r->max_screen_radius < 0 || std::isnan(r->min_opacity))
        return fail(GSR_ERR_INVALID,
                    "[gsr] %s: bad rule: grad_threshold = %g, dense_size = %g, max_world_size = %g (non-negative finite numbers), "
                    "max_screen_radius = %d (at least 0), min_opacity = %g (not NaN)",
                    who, (double)r->grad_threshold, (double)r->dense_size, (double)r->max_world_size, r->max_screen_radius,
                    (double)r->min_opacity);
    return GSR_OK;
}

static DensityRuleDev density_rule_dev(const gsr_density_rule& r)
{
    DensityRuleDev d;
    d.grad_threshold = r.grad_threshold;
    d.dense_size = r.dense_size;
    d.min_opacity = r.min_opacity;
    d.max_world_size = r.max_world_size;
    d.max_screen_radius = r.max_screen_radius;
    d.log_scales = r.log_scales != 0;
    d.normalize_rotations = r.normalize_rotations != 0;
    d.key0 = (uint32_t)(r.seed & 0xFFFFFFFFull);
    d.key1 = (uint32_t)(r.seed >> 32);
    return d;
}

size_t gsr_density_scratch_bytes(int P) { return density_sizes_ok(P) ? density_scratch_bytes(P) : 0; }

int gsr_density_plan(int P, const gsr_density_rule* rule, const float* scales, const float* opacities, const float* grad_norm_sum,
                     const int32_t* visible_views, const int32_t* max_radius, const uint8_t* prune_mask, uint32_t* offsets, uint8_t* action,
                     int64_t* totals, void* scratch, size_t scratch_bytes, gsr_stream_t stream)
{
    const char* who = "density_plan";
    if (!density_sizes_ok(P)) return fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes P=%d (at least 1, 2 P below 2^31)", who, P);
    if (int rc = density_rule_check(who, rule)) return rc;
    if (!rule || !scales || !opacities || !grad_norm_sum || !visible_views || !max_radius || !offsets || !action || !totals || !scratch)
        return fail(GSR_ERR_INVALID, "[gsr] %s: rule, scales, opacities, grad_norm_sum, visible_views, max_radius, offsets, action, totals or "
                                     "scratch is NULL", who);
    if (scratch_bytes < density_scratch_bytes(P))
        return fail(GSR_ERR_CAPACITY, "[gsr] %s: scratch too small (%zu < %zu: gsr_density_scratch_bytes(%d))", who, scratch_bytes,
                    density_scratch_bytes(P), P);
    const DensityPlanArgs a{P, scales, opacities, grad_norm_sum, visible_views, max_radius, prune_mask, offsets, action, totals,
                            reinterpret_cast<uint32_t*>(scratch)};
    const Launch L{(hipStream_t)stream, 0};
    ProfScope ps("density_plan", L.stream);
    return launch_density_plan(L, density_rule_dev(*rule), a);
}

int gsr_density_apply(int P, int G, const gsr_density_group* groups, const gsr_density_rule* rule, const uint32_t* offsets,
                      const uint8_t* action, const float* scales, const float* rotations, const float* noise, int32_t* index, int64_t P_out,
                      gsr_stream_t stream)
{
    const char* who = "density_apply";
    if (!density_sizes_ok(P)) return fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes P=%d (at least 1, 2 P below 2^31)", who, P);
    if (G < 1 || G > DENSITY_MAX_GROUPS) return fail(GSR_ERR_INVALID, "[gsr] %s: group count %d outside 1..%d", who, G, DENSITY_MAX_GROUPS);
    // (the table is read for its sizes and roles before its pointers are judged: a NULL table falls to the pointer check)
    for (int k = 0; groups && k < G; k++) {
        const gsr_density_group& s = groups[k];
        if (s.width < 1 || 2 * (int64_t)P * (int64_t)s.width >= (1ll << 31))
            return fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes in group %d: width %d (at least 1, 2 P width = 2 x %d x %d below 2^31)", who, k,
                        s.width, P, s.width);
        if (s.role < GSR_DENSITY_COPY || s.role > GSR_DENSITY_MOMENT)
            return fail(GSR_ERR_INVALID, "[gsr] %s: bad sizes in group %d: role %d is none of COPY, MEANS, SCALES, MOMENT", who, k, s.role);
    }
    int n_means = 0, n_scales = 0;
    for (int k = 0; groups && k < G; k++) {
        const gsr_density_group& s = groups[k];
        if ((s.role == GSR_DENSITY_MEANS || s.role == GSR_DENSITY_SCALES) && s.width != 3)
            return fail(GSR_ERR_INVALID, "[gsr] %s: group %d has the role %s and width %d: it takes width 3", who, k,
                        s.role == GSR_DENSITY_MEANS ? "MEANS" : "SCALES", s.width);
        n_means += s.role == GSR_DENSITY_MEANS;
        n_scales += s.role == GSR_DENSITY_SCALES;
    }
    if (n_means > 1 || n_scales > 1)
        return fail(GSR_ERR_INVALID, "[gsr] %s: %d MEANS and %d SCALES groups: at most one of each", who, n_means, n_scales);
    if (int rc = density_rule_check(who, rule)) return rc;
    if (!groups || !rule || !offsets || !action) return fail(GSR_ERR_INVALID, "[gsr] %s: groups, rule, offsets or action is NULL", who);
    for (int k = 0; k < G; k++)
        if (!groups[k].src || !groups[k].dst) return fail(GSR_ERR_INVALID, "[gsr] %s: src or dst of group %d is NULL", who, k);
    if (n_means && (!scales || !rotations))
        return fail(GSR_ERR_INVALID, "[gsr] %s: scales or rotations is NULL and a MEANS group is present", who);
    if (P_out < 0 || P_out > 2 * (int64_t)P)
        return fail(GSR_ERR_INVALID, "[gsr] %s: P_out = %lld outside 0..2 P = %lld", who, (long long)P_out, 2 * (long long)P);
    if (P_out == 0) return GSR_OK;

    DensityTable T;
    std::memset(&T, 0, sizeof(T));
    T.G = G;
    int64_t units = 0;
    for (int k = 0; k < G; k++) units += div_up(P_out * groups[k].width, DENSITY_BLOCK_ELEMS);
    uint32_t end = 0;
    for (int k = 0; k < G; k++) {
        const gsr_density_group& s = groups[k];
        DensityGroupDev& d = T.g[k];
        d.src = s.src;
        d.dst = s.dst;
        d.n = (uint32_t)(P_out * s.width);
        d.width = (uint32_t)s.width;
        d.block_end = end += density_group_blocks(d.n, units);
        d.role = s.role;
        d.vec = (s.role == GSR_DENSITY_COPY || s.role == GSR_DENSITY_MOMENT) && s.width % DENSITY_VEC == 0 &&
                (((uintptr_t)s.src | (uintptr_t)s.dst) & 15u) == 0;
    }
    const DensityApplyArgs a{P, (uint32_t)P_out, offsets, action, scales, rotations, noise, index};
    const Launch L{(hipStream_t)stream, 0};
    ProfScope ps("density_apply", L.stream);
    return launch_density_apply(L, density_rule_dev(*rule), T, a);
}

int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     gsr_stream_t stream)
{
    (void)projmatrix;
    if (P < 0) return fail(GSR_ERR_INVALID, "[gsr] P < 0");
    if (P == 0) return GSR_OK;
    if (!means3D || !viewmatrix || !present) return fail(GSR_ERR_INVALID, "[gsr] NULL pointer");
    const Launch L{(hipStream_t)stream, 0};
    return launch_mark_visible(L, P, means3D, viewmatrix, present);
}

long long gsr_d2h_count(void) { return gsr::g_d2h_count.load(); }
int gsr_set_forward_half_views(int views) { return gsr::forward_half_views(views); }
int gsr_set_backward_moments(int mode) { return gsr::backward_subquadrant_moments(mode); }
int gsr_set_render_math(int mode) { return gsr::render_math(mode); }
int gsr_set_train_math(int mode) { return gsr::train_math(mode); }

int gsr_last_list_pairs(int64_t* out, int V)
{
    if (!out || V < 0) return fail(GSR_ERR_INVALID, "[gsr] gsr_last_list_pairs: bad argument");
    for (int v = 0; v < V; v++) out[v] = (size_t)v < gsr::t_list_pairs.size() ? gsr::t_list_pairs[(size_t)v] : 0;
    return GSR_OK;
}

const char* gsr_last_error(void) { return gsr::last_error(); }
const char* gsr_version(void) { return "gsr-hip 0.3 (gfx950)"; }

}  // extern "C"
