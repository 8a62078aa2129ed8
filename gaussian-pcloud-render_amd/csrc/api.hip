// api.hip -- the C ABI of include/gsr.h: argument checks, arena carving, kernel sequencing.
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
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include <atomic>
#include <map>
#include <mutex>

namespace gsr {

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const Launch& L, const char* what)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && L.debug) e = hipStreamSynchronize(L.stream);  // CHECK_CUDA(…, debug) of the reference
    if (e != hipSuccess) return fail(GSR_ERR_HIP, "[gsr] %s: %s", what, hipGetErrorString(e));
    return GSR_OK;
}

// ---- optional per-step timing (hipEvents on the launch stream) -------------------------------------
// Records are kept PER STREAM (several host threads may render at once, each on its own stream, and one frame's forward
// and backward usually come from different host threads -- autograd runs the backward on its own thread -- but on the
// same stream).  The switch is process wide.
struct ProfEntry {
    const char* name;
    int a, b;  // indices into the stream's event pool
};
struct ProfTables {
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    std::vector<ProfEntry> rec;
    int event()
    {
        if (used == pool.size()) {
            // timing events only: no system-scope fence when they are recorded (hipEventRecord's default release writes the L2s back
            // and invalidates them between two stages, so the kernel behind an event pair started cold: the per-stage pass read
            // k_render_backward 7-10 % slower than the kernel trace of the same run, profiles/r04_bench_kernel_stats.csv)
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) (void)hipEventCreate(&e);
            pool.push_back(e);
        }
        return (int)used++;
    }
};
static std::atomic<int> g_prof_on{0};    // 0 off, 1 every stage, 2 the two render kernels only (cheap enough for a timed region)
static std::mutex g_prof_mu;
static std::map<hipStream_t, ProfTables> g_prof;   // guarded by g_prof_mu

struct ProfScope {
    hipStream_t s;
    bool on;
    ProfEntry e;
    ProfScope(const char* name, hipStream_t stream) : s(stream), on(false)
    {
        const int mode = g_prof_on;
        on = mode == 1 || (mode == 2 && strncmp(name, "render_", 7) == 0);
        if (!on) return;
        e.name = name;
        hipEvent_t ea;
        {
            std::lock_guard<std::mutex> lk(g_prof_mu);
            ProfTables& t = g_prof[s];
            e.a = t.event();
            e.b = t.event();
            ea = t.pool[e.a];
        }
        (void)hipEventRecord(ea, s);
    }
    ~ProfScope()
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(g_prof_mu);
        ProfTables& t = g_prof[s];
        (void)hipEventRecord(t.pool[e.b], s);
        t.rec.push_back(e);
    }
};

// ---- per-thread landing zone for the counter read-back ----------------------------------------------------
// Host memory mapped into the device: the pair-emission kernel stores the per-view counters there itself, and the host
// reads them after an event recorded behind that kernel.  No copy command (on this runtime a small device->host copy is a
// blit kernel plus two ~10 us bubbles in the stream).
constexpr int MAX_VIEWS = 256;
// One per (host thread, device): an event belongs to the device that was current when it was created, so a thread that
// renders on several GPUs needs one landing zone for each.
struct HostLanding {
    uint64_t* pinned = nullptr;   // [MAX_VIEWS][4]: num_rendered, trap flag, stall flag, -   (host address)
    uint64_t* mapped = nullptr;   // the same memory as the device sees it
    hipEvent_t ev = nullptr;
};
static thread_local std::map<int, HostLanding> t_lands;
static int landing(HostLanding** out)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(GSR_ERR_HIP, "[gsr] hipGetDevice: %s", hipGetErrorString(hipGetLastError()));
    HostLanding& h = t_lands[dev];
    if (!h.pinned) {
        if (hipHostMalloc((void**)&h.pinned, MAX_VIEWS * 4 * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer((void**)&h.mapped, h.pinned, 0) != hipSuccess ||
            // (hipEventDisableSystemFence on this event was tried -- the counters live in coherent host memory and the kernel fences
            // them itself, so the record would not need the system-scope release of the L2s -- and cost the per-view path a fifth of
            // its rate, 1 363 -> 1 050-1 130 frames/s, gpurun_out/r4m: waiting for such an event does not return when the emission
            // kernel ends but when the stream drains, and the host stops running ahead of the device)
            hipEventCreateWithFlags(&h.ev, hipEventDisableTiming) != hipSuccess) {
            h.pinned = nullptr;
            return fail(GSR_ERR_HIP, "[gsr] pinned host buffer: %s", hipGetErrorString(hipGetLastError()));
        }
    }
    *out = &h;
    return GSR_OK;
}

// pairs in the lists of the calling thread's last forward, per view (<= num_rendered: footprint clipping); gsr_last_list_pairs
static thread_local std::vector<int64_t> t_list_pairs;

// device->host read-backs the library has issued since it was loaded (one per forward call: the per-view counters)
static std::atomic<long long> g_d2h_count{0};

// ---- how the pair emission numbers its workgroups (common.hpp block_tickets) ------------------------------------------------------
static std::atomic<int> g_tickets{[] { const char* e = getenv("GSR_TICKETS"); return e && atoi(e) == 0 ? 0 : 1; }()};
int block_tickets(int set)
{
    if (set >= 0) g_tickets = set != 0;
    return g_tickets;
}

static int tile_count(const gsr_params* p) { return ((p->W + TILE_X - 1) / TILE_X) * ((p->H + TILE_Y - 1) / TILE_Y); }

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

// how many u32 tile-key bits the tile sort covers: the reference's 32+bit minus the 32 depth bits
static int tile_bits(int T) { return (int)higher_msb((uint32_t)T); }
// which of the two ping-pong buffers holds the sorted lists (depends on the pass count only)
static int sorted_buffer(int T) { return ((tile_bits(T) + RADIX_BITS - 1) / RADIX_BITS) & 1; }

static inline void* align256(void* p) { return (void*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

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

// What the last forward on a geometry arena saved for the backward, kept on the host so that gsr_backward_batch and
// gsr_backward_batch_channels can refuse a backward that does not match it without reading anything back from the device.  Keyed by
// the arena's address: every forward and recolor on an arena rewrites its record.
struct FrameRecord {
    int kind = 0;             // 0 colour forward, 1 channels forward, 2 recolor
    int need_backward = 0;
    int nx = 0, layout = 0;   // channels forwards
    int V = 0, P = 0, W = 0, H = 0;
    const void* xstate = nullptr;   // the extra-state block the channels forward saved into (NULL: none)
    size_t xstate_bytes = 0;
    int fwd_need_backward = -1;  // need_backward of the forward whose geometry and lists the arena holds (a recolor carries it on;
                                 // -1: unknown, a recolor on an arena without a record)
    int64_t list_pairs = -1;     // largest per-view pair count of that forward's lists (a recolor carries it on; -1: unknown): what the
                                 // scratch of a deterministic backward has to hold slots for
    int math = 0;                // arithmetic of the call that last wrote the colour saves (0 exact, 1 fast): the forward, or a recolor --
                                 // it rewrites final_T and n_contrib of every pixel and, through the same kernel, every slice-boundary
                                 // state and accumulated colour a backward reads.  The render backward runs the same mode.
    int bwd_done = 0;            // a backward has run since this record was written (every forward and recolor writes a fresh one):
                                 // the gradient records hold its sums, which is what gsr_backward_cameras reads
    FrameRecord() = default;
    FrameRecord(int kind_, const gsr_params* p, int V_) : kind(kind_), need_backward(p->need_backward != 0), V(V_), P(p->P), W(p->W), H(p->H) {}
};
static std::mutex g_frames_mu;
static std::map<const void*, FrameRecord> g_frames;
static void note_frame(const void* geom, const FrameRecord& r)
{
    std::lock_guard<std::mutex> lk(g_frames_mu);
    if (g_frames.size() > 4096 && !g_frames.count(geom)) g_frames.clear();   // (arenas come and go; records of freed ones are dropped)
    g_frames[geom] = r;
}
static bool find_frame(const void* geom, FrameRecord& r)
{
    std::lock_guard<std::mutex> lk(g_frames_mu);
    const auto it = g_frames.find(geom);
    if (it == g_frames.end()) return false;
    r = it->second;
    return true;
}
// read-modify-write of an arena's record under one lock (no record: nothing happens)
template <class F> static void update_frame(const void* geom, F change)
{
    std::lock_guard<std::mutex> lk(g_frames_mu);
    const auto it = g_frames.find(geom);
    if (it != g_frames.end()) change(it->second);
}

// The one check of an arena's record for the entries that run on the arenas of a finished forward or recolor: `who` (the entry's
// name in the messages) needs the last forward / recolor to have saved for a backward (GATE_SAVES; saves_tail ends that message),
// a backward to have run since (GATE_RECORDS), and always the same V, P, W, H -- asked in this order.  Without a record (an arena
// whose forward ran before the record table was last dropped, at more than 4096 arenas) the call goes ahead as it always did:
// refusing it would break a valid call, and the callers' contract (gsr.h) is unchanged.  Returns through `out` (may be NULL) the
// record, and through `known` whether there is one.
enum { GATE_SAVES = 1, GATE_RECORDS = 2 };
static int frame_gate(const char* who, const void* geom, const gsr_params* p, int V, int needs, const char* saves_tail,
                      FrameRecord* out = nullptr, bool* known = nullptr)
{
    FrameRecord r;
    const bool found = find_frame(geom, r);
    if (out) *out = r;
    if (known) *known = found;
    if (!found) return GSR_OK;
    if ((needs & GATE_SAVES) && !r.need_backward)
        return fail(GSR_ERR_INVALID, "[gsr] %s: the last %s on this geometry arena had need_backward = 0%s", who,
                    r.kind == 2 ? "gsr_forward_recolor" : "forward", saves_tail);
    if ((needs & GATE_RECORDS) && !r.bwd_done)
        return fail(GSR_ERR_INVALID, "[gsr] %s: no backward has run since the last forward or recolor on this geometry arena (the "
                    "gradient records are empty; run one of the gsr_backward entries first)", who);
    if (r.V != V || r.P != p->P || r.W != p->W || r.H != p->H)
        return fail(GSR_ERR_INVALID, "[gsr] %s: V = %d, P = %d, %d x %d, but the last forward or recolor on this geometry arena "
                    "had V = %d, P = %d, %d x %d", who, V, p->P, p->W, p->H, r.V, r.P, r.W, r.H);
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

// ---- inspection (tests / roofline report only) -------------------------------------------------------
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

void gsr_set_profiling(int on)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on < 0 ? 0 : on > 2 ? 1 : on;
    for (auto& kv : g_prof) { kv.second.rec.clear(); kv.second.used = 0; }
}

int gsr_get_profile(const char** names, float* ms, int cap)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int n = 0;
    for (auto& kv : g_prof) {
        ProfTables& t = kv.second;
        for (auto& e : t.rec) {
            if (n >= cap) break;
            (void)hipEventSynchronize(t.pool[e.b]);
            float d = 0;
            (void)hipEventElapsedTime(&d, t.pool[e.a], t.pool[e.b]);
            names[n] = e.name;
            ms[n] = d;
            n++;
        }
        t.rec.clear();
        t.used = 0;
    }
    return n;
}

#ifdef GSR_STATS
__attribute__((visibility("default"))) int gsr_debug_bwd_stats(unsigned long long* out8, int reset) { return gsr::debug_bwd_stats(out8, reset); }
__attribute__((visibility("default"))) int gsr_debug_scatter_times(unsigned long long* out8, int reset) { return gsr::debug_scatter_times(out8, reset); }
__attribute__((visibility("default"))) int gsr_debug_fwd_times(unsigned long long* out8, int reset) { return gsr::debug_fwd_times(out8, reset); }
__attribute__((visibility("default"))) int gsr_debug_fwd_records(unsigned* out, int n) { return gsr::debug_fwd_records(out, n); }
__attribute__((visibility("default"))) int gsr_debug_bwd_times(unsigned long long* out8, int reset) { return gsr::debug_bwd_times(out8, reset); }
__attribute__((visibility("default"))) int gsr_debug_bwd_records(unsigned* out, int n) { return gsr::debug_bwd_records(out, n); }
__attribute__((visibility("default"))) int gsr_debug_dup_times(unsigned long long* out8, int reset) { return gsr::debug_dup_times(out8, reset); }
#endif

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

const char* gsr_last_error(void) { return gsr::g_err; }
const char* gsr_version(void) { return "gsr-hip 0.3 (gfx950)"; }

}  // extern "C"
