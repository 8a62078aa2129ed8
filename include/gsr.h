/*
 * gsr.h -- C ABI of the MI355X-native Gaussian tile rasterizer (libgsr_hip.so).
 *
 * This is the drop-in boundary for the one hot path of huzi96/gaussian-pcloud-render:
 * the differentiable rasterizer behind diff_gaussian_rasterization.GaussianRasterizer.
 * It replaces the reference's torch/pybind binding + CUDA core:
 *
 *   reference (under /root/reference/diff-gaussian-rasterization/)      this header
 *   ------------------------------------------------------------------  -------------------------
 *   ext.cpp:16  rasterize_gaussians        -> rasterize_points.cu:35   gsr_forward_stage1 + _stage2
 *               CudaRasterizer::Rasterizer::forward  rasterizer.h:35-59
 *   ext.cpp:17  rasterize_gaussians_backward -> rasterize_points.cu:117 gsr_backward
 *               CudaRasterizer::Rasterizer::backward rasterizer.h:61-90
 *   ext.cpp:18  mark_visible               -> rasterize_points.cu:198  gsr_mark_visible
 *               CudaRasterizer::Rasterizer::markVisible rasterizer.h:28-33
 *   rasterizer_impl.h:65-72 required<GeometryState/ImageState/BinningState>()
 *                                                                       gsr_geom_bytes / gsr_image_bytes / gsr_binning_bytes
 *   auxiliary.h:166-173 CHECK_CUDA(..., debug) + thrown runtime_error   int status + gsr_last_error()
 *
 * Conventions
 *   - plain C: raw device pointers, ints, floats; no torch / ATen / pybind types.
 *   - the CALLER owns every buffer (inputs, outputs, the three opaque scratch arenas); the library
 *     never allocates device memory on the hot path.  Arena contents are private to the library
 *     (struct-of-arrays) and only need to survive from forward to backward, exactly
 *     like geomBuffer/binningBuffer/imgBuffer in diff_gaussian_rasterization/__init__.py:97.
 *   - optional inputs are NULL when absent (the reference passes data_ptr() of empty tensors, i.e.
 *     nullptr: rasterizer_impl.cu:321,389,411).
 *   - every launch goes to the explicit `stream` (the reference uses the legacy default stream).
 *   - the binning arena size depends on num_rendered, which the reference reads back in the middle of
 *     the frame to grow its arena through a std::function callback (rasterizer_impl.cu:279-285).  Here
 *     the count stays on the device: the caller hands over an arena of some CAPACITY (gsr_binning_bytes
 *     of the pair count it expects, e.g. the previous frame's plus slack), the whole frame is enqueued
 *     without a host round trip, and gsr_forward_batch reports afterwards whether the capacity was enough
 *     (GSR_RETRY: allocate gsr_binning_bytes(max num_rendered) and repeat with resume = 1).  The
 *     two-stage pair gsr_forward_stage1/_stage2 keeps the reference's synchronous shape on top of that.
 *   - a call covers a batch of V camera views of ONE cloud (V = 1: the reference's per-view call).
 *     Per-view inputs (viewmatrix, projmatrix, campos) and outputs (radii, out_color, dL_dpix) are V
 *     consecutive arrays; each scratch arena is V times the single-view size.
 *   - return value: 0 = ok, negative = error (text via gsr_last_error()), GSR_RETRY = see above.  With
 *     debug != 0 the library synchronises and checks after every kernel like CHECK_CUDA(…, true).
 */
#ifndef GSR_H
#define GSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_ERR_INVALID (-1)  /* bad argument (message says which)                              */
#define GSR_ERR_HIP (-2)      /* a HIP call or kernel failed                                    */
#define GSR_ERR_CAPACITY (-3) /* an arena is smaller than gsr_*_bytes() requires                */
#define GSR_ERR_TRAP (-4)     /* prefiltered=1 but a point was culled (auxiliary.h:156-160)     */
#define GSR_RETRY 1           /* forward: a view produced more pairs than the binning arena holds */

typedef void* gsr_stream_t; /* hipStream_t */

/* Arguments shared by forward and backward: the 19/21-argument lists of
 * diff_gaussian_rasterization/__init__.py:60-80,109-129 minus the tensors' metadata. */
typedef struct gsr_params {
    int P;                 /* number of Gaussians (means3D.size(0))                                  */
    int D;                 /* active SH degree (raster_settings.sh_degree)                           */
    int M;                 /* SH coefficients per Gaussian = sh.size(1), 0 when shs is absent        */
    int W, H;              /* image_width, image_height                                              */
    float tanfovx, tanfovy;
    float scale_modifier;
    int prefiltered;
    int debug;
    int need_backward;     /* 0: inference call, skip the saves only gsr_backward reads (SH clamp mask,
                              accumulated colour, per-pixel state at the list-slice boundaries the backward's
                              work items start from: every 512 entries of a tile's list in single-view
                              submissions, every 1024 from two views per submission on);
                              gsr_backward is only valid after a forward with need_backward = 1      */
    int reference_lists;   /* 0 (default): a Gaussian emits pairs for the tiles of the reference's rectangle
                              (auxiliary.h:46-56) in which alpha can reach 1/255 -- the rectangle clipped to the
                              bounding box of the ellipse  d^T conic d <= 2 log(255 opacity), conservatively against
                              fp32 rounding (csrc/tile_cull.hpp).  The reference evaluates the other tiles' entries
                              and skips them at every pixel (forward.cu:336-347), so out_color, radii, num_rendered
                              and every gradient are the same bit for bit / sum for sum; only the PRIVATE lists
                              (and the list positions in n_contrib) differ.  1: the reference's full rectangles --
                              lists, ranges and n_contrib identical to the reference's (parity tests).
                              (occupies what used to be padding: zero-initialised callers are unaffected)  */
    const float* bg;             /* [3]        device */
    const float* means3D;        /* [P,3]      device */
    const float* shs;            /* [P,M,3]    device or NULL */
    const float* colors_precomp; /* [P,3]      device or NULL */
    const float* opacities;      /* [P]        device */
    const float* scales;         /* [P,3]      device or NULL */
    const float* rotations;      /* [P,4]      device or NULL */
    const float* cov3D_precomp;  /* [P,6]      device or NULL */
    const float* viewmatrix;     /* [V][16] column-major when flattened (auxiliary.h:58-76) device */
    const float* projmatrix;     /* [V][16]    device */
    const float* campos;         /* [V][3]     device */
} gsr_params;

/* Scratch arena sizes in bytes for ONE view (256-B aligned sub-arrays inside); a batch of V views needs V times as much.
 * gsr_binning_bytes(n) is an arena that holds n pairs per view: the library derives the capacity from the arena's size.
 * The arena contract.  Arenas (and the extra-state block of the channels calls) need NOT be initialised: any bytes will do,
 * the bytes of an earlier frame included -- the usual state in a training loop, where every frame renders into the allocation of
 * the one before.  What they hold between calls is the library's: a caller neither reads nor changes it between a forward and the
 * calls that follow it on the same arenas.  No result of a call depends on what the arenas held BEFORE the forward (or the stage
 * pair) that starts a frame: every output, private list and gradient is the one the same calls give on zero-filled arenas, bit for
 * bit wherever this header promises repeatable bits, with another V, another need_backward, another arithmetic mode or another
 * kind of call (colour, channels, recolor, a retried and resumed frame) before it (tests/test_gpu_arena_state.py; which kernel writes
 * and reads which part under which condition: DESIGN.md section 6). */
size_t gsr_geom_bytes(int P);
/* The geometry arena of a call with need_backward = 0 (inference): without the 64-B per-Gaussian gradient records that only
 * the backward accumulates into (they follow the V per-view arenas inside the allocation, so the layout of everything else
 * does not depend on the flag).  A forward with need_backward = 1 and every backward need V * gsr_geom_bytes(P). */
size_t gsr_geom_bytes_inference(int P);
size_t gsr_image_bytes(int W, int H);
size_t gsr_binning_bytes(int64_t num_rendered);

/* Forward of V views in one submission (rasterize_points.cu:35-115 / Rasterizer::forward rasterizer.h:35-59, looped over
 * views by the reference's caller, simple_raw_render.py:259-278): per-Gaussian preprocess (cull, EWA projection, SH colour),
 * depth ordering, (tile, Gaussian) pair emission in depth order with its prefix sum, stable radix sort by tile, tile
 * ranges, per-tile front-to-back alpha compositing.  Writes radii[V,P], out_color[V,3,H,W] (planar CHW per view) and
 * num_rendered[V] (HOST array): the number of (tile, Gaussian) pairs of the reference's tile rectangles, i.e. exactly the
 * reference's num_rendered (rasterizer_impl.cu:277-281).  The lists the library keeps hold at most that many pairs (fewer
 * with footprint clipping, see gsr_params.reference_lists; gsr_last_list_pairs reports how many).
 * Nothing on the host waits for the device until every kernel of the batch is enqueued.
 * Returns GSR_OK, or GSR_RETRY when some view's lists exceed the per-view capacity of `binning`: out_color is then
 * invalid; call again with resume = 1, the same geom / image arenas and a binning arena of at least
 * V * gsr_binning_bytes(n) bytes, n = max_v num_rendered[v] (always enough) or max_v of gsr_last_list_pairs (exact)
 * (only the binning half of the frame is repeated). */
int gsr_forward_batch(const gsr_params* p, int V, void* geom, size_t geom_bytes, void* image, size_t image_bytes,
                      void* binning, size_t binning_bytes, int* radii, float* out_color, int64_t* num_rendered,
                      int resume, gsr_stream_t stream);

/* gsr_forward_batch that also composites `nx` (4 or 8; pad with zero channels) extra per-Gaussian channels with the SAME alphas,
 * transmittances and stopping decisions as the colour: out_extra[v][k] = sum_i extra[v][i][k] * view_scale[v][k] * alpha_i * T_i +
 * T_final * bg_extra[k], term for term what a separate call with colors_precomp = those channels would produce -- the
 * reference's callers render world xyz, a hit map and normals that way, one full rasterizer call each
 * (simple_raw_render.py:410-524), recomputing identical alphas four times.  extra_per_view = 0: extra [P][nx] is shared by the
 * views; 1: extra [V][P][nx], one array per view (the reference turns every normal towards the camera of the view it renders,
 * simple_raw_render.py:264-268); 2 (nx = 8 only): split -- extra holds channels 0..3 as [P][4] shared by the views, followed by
 * channels 4..7 as [V][P][4] (world xyz + hit value once, the turned normals per view: half the memory of 1 for that use).  extra_view_scale [V][nx] (or NULL) multiplies the values per view and channel.
 * out_extra is [V][nx][H][W].  P == 0: nothing is written (like out_color).  Same GSR_RETRY / resume contract. */
int gsr_forward_batch_channels(const gsr_params* p, int V, void* geom, size_t geom_bytes, void* image, size_t image_bytes,
                               void* binning, size_t binning_bytes, int* radii, float* out_color, int64_t* num_rendered, int resume,
                               int nx, int extra_per_view, const float* extra, const float* extra_view_scale, const float* bg_extra,
                               float* out_extra, gsr_stream_t stream);

/* Training with the extra channels.  gsr_forward_batch_channels_train is gsr_forward_batch_channels that, with p->need_backward = 1,
 * also saves into the caller-owned block `extra_state` what the channels backward needs beyond the colour's saves: the extra
 * channels accumulated per pixel at the list-slice boundaries and at the end of the walk.  Outputs are bit-identical to
 * gsr_forward_batch_channels.  The block holds at least V * gsr_extra_state_bytes(W, H, n, nx) + 256 bytes, n being the pair count
 * the binning arena was sized for (V * gsr_binning_bytes(n) bytes; after a GSR_RETRY both grow together and the resumed call saves
 * into the new block); gsr_geom_bytes / gsr_image_bytes / gsr_binning_bytes are unchanged.  With need_backward = 0 the block is
 * not touched.  The library remembers, per geometry arena, what the last forward or recolor on it saved, so that the backward can
 * refuse a mismatch without reading anything back from the device. */
size_t gsr_extra_state_bytes(int W, int H, int64_t num_rendered, int nx);
int gsr_forward_batch_channels_train(const gsr_params* p, int V, void* geom, size_t geom_bytes, void* image, size_t image_bytes,
                                     void* binning, size_t binning_bytes, int* radii, float* out_color, int64_t* num_rendered,
                                     int resume, int nx, int extra_per_view, const float* extra, const float* extra_view_scale,
                                     const float* bg_extra, float* out_extra, void* extra_state, size_t extra_state_bytes,
                                     gsr_stream_t stream);

/* The reference's synchronous shape for one view.  Stage 1: preprocess, depth ordering, pair counting; returns
 * num_rendered through *num_rendered_out after a device->host read-back on `stream` (cf. rasterizer_impl.cu:281).
 * out_color is not touched. */
int gsr_forward_stage1(const gsr_params* p, void* geom, size_t geom_bytes, void* image, size_t image_bytes,
                       int* radii, int64_t* num_rendered_out, gsr_stream_t stream);

/* Stage 2: pair emission, sort, ranges, compositing into out_color[3,H,W], with a binning arena of at least
 * gsr_binning_bytes(num_rendered) bytes. */
int gsr_forward_stage2(const gsr_params* p, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes,
                       void* image, size_t image_bytes, int64_t num_rendered, float* out_color, gsr_stream_t stream);

/* Colour-only re-render.  The reference's caller renders four passes per view that differ only in the
 * per-Gaussian colour (world xyz / SH colour / ones / normals, simple_raw_render.py:410-524), each through the whole
 * pipeline.  After a forward this entry re-renders the same V views with other colours on the SAME geometry, lists and
 * ranges: p->colors_precomp (verbatim; [P,3] shared by the views, or [V,P,3] with colors_per_view != 0 -- the reference's
 * normal pass flips the normals' sign per view) or p->shs (evaluated like the forward does); only P, D, M, W, H, bg, means3D,
 * shs / colors_precomp, campos of *p are read.  The result is bit-identical to a full forward with those colours.  The
 * arenas stay valid for further recolor calls.  With p->need_backward = 1 (and arenas of a need_backward forward) the
 * saves the backward reads are rewritten too (per-pixel state at the list-slice boundaries, accumulated colour, SH clamp
 * mask), so a backward afterwards -- called with the SAME colour inputs -- differentiates the LAST colours rendered; with
 * need_backward = 0 a backward after the recolor is not supported (gsr_backward_batch refuses it).  A backward after a
 * colors_per_view recolor is called with colors_precomp = the [V,P,3] colours and returns dL_dcolor [P,3] SUMMED over the views
 * (like every per-Gaussian gradient); gsr_backward_view_stats after that backward separates the per-view shares (dL_dcolor_views). */
int gsr_forward_recolor(const gsr_params* p, int V, int colors_per_view, void* geom, size_t geom_bytes, const void* binning,
                        size_t binning_bytes, void* image, size_t image_bytes, float* out_color, gsr_stream_t stream);

/* Backward of a batch (rasterize_points.cu:117-196 / Rasterizer::backward rasterizer.h:61-90), on the arenas of ONE forward call and with
 * that call's V (the arenas' internal layout -- per-view strides, the length of the list slices whose boundary states the forward
 * saved -- follows from V; a forward batch cannot be split into several backward calls).  dL_dpix is [V,3,H,W]; the
 * per-Gaussian gradients are SUMMED over the V views (what autograd does with the reference's per-view calls on a shared
 * cloud).  Every output is written for every Gaussian (zeros where it is invisible; all M rows of dL_dsh), so nothing has
 * to be cleared by the caller -- the reference zero-fills nine tensors per call (rasterize_points.cu:151-159) -- except
 * dL_dscale / dL_drot, which are not touched when cov3D_precomp is given.  The reference's internal dL_dconic accumulator
 * lives in the geometry arena.  Valid after a forward with need_backward = 1 on the same arenas, any number of times: every
 * call returns the gradients of ITS dL_dpix (a repeated call first clears what the previous one accumulated).  GSR_ERR_INVALID with
 * a message when the library's record of the last forward or recolor on `geom` shows that it saved nothing (need_backward = 0),
 * that it was a need_backward recolor on the arenas of a need_backward = 0 forward, or that V, P, W or H differ from this call's
 * (arenas without a record -- the record table is dropped once it holds more than 4096 arenas -- are not checked).  After
 * gsr_forward_batch_channels_train with need_backward = 1 this call is valid and differentiates the COLOUR image alone (the
 * extra channels' dL_dextra taken as zero): the channels forward writes the colour's saves exactly as the colour forward does.
 * shapes: radii[V,P] dL_dmean2D[P,3] dL_dopacity[P,1] dL_dcolor[P,3] dL_dmean3D[P,3] dL_dcov3D[P,6] dL_dsh[P,M,3]
 * dL_dscale[P,3] dL_drot[P,4].
 * Alignment: dL_drot must be 16-byte aligned (GSR_ERR_INVALID otherwise); the other gradient outputs should be -- every
 * hipMalloc / torch allocation is -- because their rows then leave the kernel as whole 16-byte chunks; an output that is only
 * float-aligned is still written correctly, through slower per-row stores. */
int gsr_backward_batch(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                       size_t binning_bytes, const void* image, size_t image_bytes, const float* dL_dpix, float* dL_dmean2D,
                       float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                       float* dL_dscale, float* dL_drot, gsr_stream_t stream);

/* Deterministic colour backward (opt-in; replaces rasterize_points.cu:117-196 like gsr_backward_batch, and with it the reference's own
 * float atomics, backward.cu:523-554, whose order of arrival makes its gradients differ in their last bits from run to run; the
 * reference has no repeatable path).  gsr_backward_batch's arguments, outputs and refusals, plus a caller-owned scratch block.
 * For the same inputs, the same call shape (V, image size, moments mode, reference_lists), the same arithmetic mode (gsr_set_train_math:
 * that of the forward or recolor that wrote the saves), the same library build and the same device model, every gradient is BIT-IDENTICAL from call to call and from process to process: whichever workgroup takes which work
 * unit, whatever runs beside it.  It is NOT promised across different V (the list slices and their start states differ), builds or
 * device models.  The values are those of gsr_backward_batch up to the order of float additions: the same partial sums per (list
 * entry, 8 x 8 quadrant), stored into slots of their own instead of added with atomics, then added per Gaussian in a fixed order --
 * tile, then depth inside the tile, then quadrant.  Valid after gsr_forward_batch, after gsr_forward_recolor
 * with need_backward = 1 and after gsr_forward_batch_channels_train (it then differentiates the colour image alone), any number of
 * times over one forward, in all three moments modes.  No device->host read-back; the library allocates nothing on the device.
 *
 * gsr_backward_det_bytes(V, P, W, H, pairs) is the size of the scratch block, a pure host function: `pairs` is the largest per-view
 * pair count of the forward's lists -- max_v gsr_last_list_pairs after the forward (exact), or anything larger such as the count the
 * binning arena was sized for.  A block smaller than the forward's lists need returns GSR_ERR_CAPACITY with the needed size in the
 * message (the library remembers the lists' extent with the geometry arena's record).  The block is large: about 276 bytes per pair
 * and view (a 64-B slot per quadrant, the sort's ping-pong buffers and a flag word), i.e. 2.0 GB per view for lists of 7.3 M pairs
 * and 24 GB for 12 such views, of which only the entries the forward consumed (about 1.1 M per view there) are ever touched.
 *
 * The channels backward has a deterministic counterpart of its own, gsr_backward_batch_channels_det below. */
size_t gsr_backward_det_bytes(int V, int P, int W, int H, int64_t pairs);
int gsr_backward_batch_det(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                           size_t binning_bytes, const void* image, size_t image_bytes, const float* dL_dpix, float* dL_dmean2D,
                           float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                           float* dL_dscale, float* dL_drot, void* det_scratch, size_t det_scratch_bytes, gsr_stream_t stream);

/* Backward of gsr_forward_batch_channels_train (need_backward = 1): gsr_backward_batch's arguments and outputs -- the mean2D, conic
 * and opacity gradients now carry the extra channels' share of dL/d alpha (d = c . dL_dpix + e . dL_dextra with
 * e_k = extra_k * view_scale_k; background term T_final (bg . dL_dpix + bg_extra . dL_dextra)) -- plus dL_dextra [V][nx][H][W]
 * and dL_dextra_values, dL/d extra in the layout of `extra` (extra_per_view 0: [P][nx] summed over the views; 1: [V][P][nx];
 * 2: [P][4] summed over the views, then [V][P][4]): view_scale_k * sum over pixels of alpha T dL_dextra_k.  nx, extra_per_view,
 * extra, extra_view_scale, bg_extra and extra_state are the forward's.  Every element of dL_dextra_values is written (the library
 * clears it and accumulates into it); bg_extra and extra_view_scale get no gradient.  GSR_ERR_INVALID with a message when the
 * last forward on `geom` was not a channels forward with need_backward = 1 into this extra_state, when nx or the layout differ
 * from that forward's, or after a gsr_forward_recolor on the arenas (not supported). */
int gsr_backward_batch_channels(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                                size_t binning_bytes, const void* image, size_t image_bytes, const float* dL_dpix, float* dL_dmean2D,
                                float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                                float* dL_dscale, float* dL_drot, int nx, int extra_per_view, const float* extra,
                                const float* extra_view_scale, const float* bg_extra, const void* extra_state, size_t extra_state_bytes,
                                const float* dL_dextra, float* dL_dextra_values, gsr_stream_t stream);

/* Deterministic channels backward (opt-in): gsr_backward_batch_channels's arguments, outputs and refusals -- checked in the same
 * order with the same texts: the arena's record, the pointers, the extra-state size -- plus a caller-owned scratch block, checked
 * last (GSR_ERR_CAPACITY with the needed size and the arguments of the size query in the message).  The contract is
 * gsr_backward_batch_det's, for all outputs including dL_dextra_values: for the same inputs, the same call shape (V, image size, nx,
 * extra_per_view, moments mode, reference_lists), the same library build and the same device model every output is BIT-IDENTICAL
 * from call to call and from process to process; not promised across different V, builds or device models.  The values are those of
 * gsr_backward_batch_channels up to the order of float additions.  One kernel stores the colour / geometry sums (which carry the
 * extras' share) AND dL/d extra of every (list entry, 8 x 8 quadrant) into slots of their own; no float atomic is issued anywhere.
 * Order of the additions, for the gradient records and for dL/d extra alike: per view and Gaussian, the entries of the Gaussian in
 * the view's lists by tile, then by depth inside the tile, then the quadrants 0, 1, 2, 3 of the tile; quadrants the kernel did not
 * evaluate are left out; the running sum is kept in float64 and rounded to float32 ONCE per view.  Rows of dL_dextra_values that
 * belong to one view (extra_per_view = 1; channels 4..7 of extra_per_view = 2) are that rounded value.  Rows the views share
 * (extra_per_view = 0; channels 0..3 of extra_per_view = 2) are the per-view float32 values added for view 0, 1, .. V - 1 in
 * float64 and rounded to float32 once more.  Rows of Gaussians that no evaluated entry reached are exactly zero.  Valid after
 * gsr_forward_batch_channels_train with need_backward = 1, any number of times over one forward (not after gsr_forward_recolor), in
 * all three moments modes.  No device->host read-back; the library allocates nothing on the device.
 *
 * gsr_backward_det_channels_bytes(V, P, W, H, pairs, nx, extra_per_view) is the size of the scratch block, a pure host function;
 * `pairs` as for gsr_backward_det_bytes.  It is gsr_backward_det_bytes(V, P, W, H, pairs) plus the extras' slots -- 16 nx bytes per
 * pair and view (64 B for nx = 4, 128 B for nx = 8: about 340 / 404 bytes per pair and view in all) -- plus the staging of the shared
 * rows, 4 V P nx bytes (extra_per_view = 0) or 16 V P bytes (extra_per_view = 2).  0 for arguments gsr_backward_det_bytes answers
 * with 0 and for an nx / extra_per_view pair the channels forward refuses. */
size_t gsr_backward_det_channels_bytes(int V, int P, int W, int H, int64_t pairs, int nx, int extra_per_view);
int gsr_backward_batch_channels_det(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, const void* binning,
                                    size_t binning_bytes, const void* image, size_t image_bytes, const float* dL_dpix, float* dL_dmean2D,
                                    float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                                    float* dL_dscale, float* dL_drot, int nx, int extra_per_view, const float* extra,
                                    const float* extra_view_scale, const float* bg_extra, const void* extra_state,
                                    size_t extra_state_bytes, const float* dL_dextra, float* dL_dextra_values, void* det_scratch,
                                    size_t det_scratch_bytes, gsr_stream_t stream);

/* One view, the reference's argument shape (num_rendered is not needed: the lists' extent lives in the arenas). */
int gsr_backward(const gsr_params* p, const int* radii, int64_t num_rendered, const void* geom, size_t geom_bytes,
                 const void* binning, size_t binning_bytes, const void* image, size_t image_bytes,
                 const float* dL_dpix /* [3,H,W] */, float* dL_dmean2D, float* dL_dopacity,
                 float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                 float* dL_drot, gsr_stream_t stream);

/* Camera gradients: dL/d viewmatrix, dL/d projmatrix and dL/d campos of every view, for pose refinement.  A separate call that runs
 * AFTER a backward on the same arenas -- gsr_backward_batch, gsr_backward_batch_det, gsr_backward, gsr_backward_batch_channels or
 * gsr_backward_batch_channels_det -- with that backward's p, V and radii; it differentiates what that backward differentiated (after
 * a channels backward the mean2D and conic sums carry the extras' share, so the result is that of colour plus channels).  It reads
 * the per-view gradient records the backward left behind the geometry arenas, pushes them through the projection chain to the camera
 * operands and adds over the Gaussians of each view; the backward's own outputs are not needed and nothing in
 * the arenas is changed, so the call may be repeated.
 *   dL_dviewmatrix, dL_dprojmatrix  [V][16] in the flattening of viewmatrix / projmatrix themselves
 *   dL_dcampos                      [V][3]: through the SH view direction; +0 with colors_precomp and at SH degree 0
 * All 35 floats of every view are written.  The entries the forward never reads are written as +0: viewmatrix[3, 7, 11, 15] and
 * projmatrix[2, 6, 10, 14] (preprocess uses rows 0, 1, 3 of the projection only).  A view in which nothing is visible gets 35 zeros.
 * Conventions: the reference's backward treats the frustum clamp of the view-space mean (|x / z| > 1.3 tanfov) as dL/dt_x = 0 (t_y
 * likewise) with the clamped t_x, t_y as constants in dL/dt_z; the camera gradient keeps that convention, so that
 *   sum_i dL_dmean3D[i][j] = sum_v ( sum_k view[k + 4j] dL_dview[12 + k] + sum_{k in 0,1,3} proj[k + 4j] dL_dproj[12 + k] - dL_dcampos[j] )
 * holds (a translation of the cloud is a translation of every camera).  Depth order, culling, radii and the tile lists are not
 * differentiated (piecewise constant), nor are tanfovx / tanfovy (intrinsics reach the image through projmatrix).
 * The terms through the 2D covariance are evaluated in float64 from the float32 inputs and records (a splat next to the camera makes
 * them cancel several hundredfold), the others in float32; every per-Gaussian term is added in float64 in a fixed order (Gaussian index inside a thread, a fixed tree
 * over the workgroup, the workgroups' partial sums by index in a second launch), rounded to float32 once: no atomics, so the result
 * is a function of the records alone -- bit-reproducible after gsr_backward_batch_det / _channels_det, and the same bits again when
 * the call is repeated over one backward.  No device->host read-back; the library allocates nothing on the device.
 *
 * scratch: caller-owned, at least gsr_camera_grad_bytes(V, P) bytes (a pure host function: 256 B per 1024 Gaussians and view, a
 * positive multiple of 256 that does not decrease with V or P; 0 for V < 1, V > 256 or P < 0); every word read is written first.
 * Checks, in this order: the parameters (as every entry); P == 0 -> GSR_OK, nothing written; a NULL radii, geom, output or scratch
 * -> GSR_ERR_INVALID; a scratch block that is too small -> GSR_ERR_CAPACITY with the needed size in the message; then the arena's
 * record -> GSR_ERR_INVALID when the last forward or recolor on `geom` had need_backward = 0, when no backward has run since it, or
 * when V, P, W or H differ from it (the outputs are then untouched).  An arena without a record is not checked. */
size_t gsr_camera_grad_bytes(int V, int P);
int gsr_backward_cameras(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes,
                         float* dL_dviewmatrix /* [V][16] */, float* dL_dprojmatrix /* [V][16] */, float* dL_dcampos /* [V][3] */,
                         void* scratch, size_t scratch_bytes, gsr_stream_t stream);

/* Density-control statistics and per-view gradients of a view batch.  Every backward returns the per-Gaussian gradients SUMMED over
 * the V views; adaptive density control (split / clone / prune) wants, per Gaussian, the sum over the views of the NORM of the
 * screen-space gradient -- which is not the norm of the sum: gradients from opposite views cancel inside dL_dmean2D --, the number
 * of views that saw the Gaussian and its largest screen radius; per-view appearance wants the colour and opacity gradients view by
 * view.  A separate call that runs AFTER a backward on the same arenas -- gsr_backward_batch, gsr_backward_batch_det, gsr_backward,
 * gsr_backward_batch_channels or gsr_backward_batch_channels_det, in either arithmetic mode -- with that backward's p, V and radii.
 * It reads radii and the per-view gradient records the backward left behind the geometry arenas and changes
 * nothing in the arenas, so it may be repeated, and may come before or after gsr_backward_cameras.  With (gx, gy) the record's
 * mean2D words of Gaussian i in view v (pixel units, like dL_dmean2D):
 *   grad_norm_sum[i] = sum_{v = 0 .. V-1} sqrt(gx^2 + gy^2): every term and the running sum in float64 from the float32 words, views
 *                      ascending, rounded to float32 once; a view in which the Gaussian is invisible or unreached adds an exact zero
 *   visible_views[i] = the number of views with radii[v][i] > 0
 *   max_radius[i]    = max_v radii[v][i], 0 when the Gaussian is visible nowhere
 * accumulate = 0 overwrites the three; accumulate != 0 updates the caller's running values in place, what a trainer keeps between two
 * densification steps: grad_norm_sum[i] = float32(double(old) + sum), visible_views[i] += count, max_radius[i] = max(old, new).
 *   dL_dmean2D_views [V][P][2], dL_dcolor_views [V][P][3], dL_dopacity_views [V][P]: the record's words of every Gaussian and view,
 *   bit for bit, zeros where nothing was accumulated; ALWAYS overwritten (accumulate does not apply to them).
 * Adding the shares in float32 for v = 0, 1, .. V-1, starting from +0, reproduces the backward's dL_dmean2D[:, 0:2], dL_dcolor and
 * dL_dopacity bit for bit: that is the order in which the backward adds them.  After a colors_per_view recolor plus backward,
 * dL_dcolor_views[v] is the gradient of view v's own colours.  After a channels backward the mean2D and opacity shares carry the extra
 * channels' part, like the summed outputs.  Each of the six outputs may be NULL (not all of them); a call for the statistics alone
 * reads 16 B of every record, one with grad_norm_sum = NULL and no shares reads radii only.  One kernel, one thread per Gaussian: no
 * atomics, no scratch, no device->host read-back, no allocation; the result is a function of the records and radii alone --
 * bit-reproducible after gsr_backward_batch_det / _channels_det, and the same bits again when the call is repeated.
 * Checks, in this order: the parameters (as every entry); P == 0 -> GSR_OK, nothing written; a NULL radii or geom -> GSR_ERR_INVALID;
 * all six outputs NULL -> GSR_ERR_INVALID; dL_dmean2D_views not 8-byte aligned -> GSR_ERR_INVALID (its rows leave as 8-byte stores);
 * then the arena's record -> GSR_ERR_INVALID when the last forward or recolor on `geom` had need_backward = 0, when no backward has
 * run since it, or when V, P, W or H differ from it (the outputs are then untouched; an arena without a record is not checked); then
 * the size of the geometry allocation (GSR_ERR_CAPACITY). */
int gsr_backward_view_stats(const gsr_params* p, int V, const int* radii, const void* geom, size_t geom_bytes, int accumulate,
                            float* grad_norm_sum /* [P] or NULL */, int* visible_views /* [P] or NULL */,
                            int* max_radius /* [P] or NULL */, float* dL_dmean2D_views /* [V][P][2] or NULL */,
                            float* dL_dcolor_views /* [V][P][3] or NULL */, float* dL_dopacity_views /* [V][P] or NULL */,
                            gsr_stream_t stream);

/* Per-Gaussian contribution statistics of a view batch: what importance-based pruning and compaction rank a Gaussian by.  One
 * read-only walk of the lists of the last forward (gsr_forward_batch, gsr_forward, the stage pair, a channels forward) or
 * gsr_forward_recolor on the same arenas, with that call's V, P, W and H -- valid with either value of need_backward, before or after
 * a backward, any number of times: it reads the projected splat records, the sorted tile lists and the ranges, and writes nothing
 * into the arenas (not the consumed-entry counts, not the gradient records, none of a backward's saves).  It composites front to back
 * exactly like the exact-mode forward: an entry with power > 0 or alpha < 1/255 is skipped, the entry with T (1 - alpha) < 1e-4 stops
 * its pixel and is not blended, pixels outside the image do not exist.  The arithmetic is ALWAYS the exact mode's, whatever
 * gsr_set_render_math and gsr_set_train_math say.  With T the transmittance in front of entry i at a pixel, w = alpha T its blend
 * weight there, and m the pixel's weight -- pixel_weights[v][y][x], or 1 without a map; a value with !(m > 0) (zero, negative, NaN)
 * is 0, and a pixel with m = 0 is left out of all four statistics (a mask):
 *   weight_sum[i]     = the sum over the (view, pixel) contributions of Gaussian i of w m
 *   weight_max[i]     = the largest w m among them (0 without a contribution)
 *   pixel_count[i]    = their number, unweighted
 *   dominant_count[i] = the number of (view, pixel) at which i has the largest unweighted w (strictly: the front-most entry wins a tie;
 *                       a pixel nothing contributes to counts for nobody)
 * radii ([V][P], may be NULL) is not read: a Gaussian with radii[v][i] == 0 is in no list of view v and gets zeros from it.
 * accumulate = 0 clears the requested outputs first, on the stream; accumulate != 0 keeps the caller's running values: weight_sum and
 * the two counts are added to, weight_max becomes the maximum of old and new (the old values are non-negative floats).  Each of the
 * four outputs may be NULL (not all of them).  One kernel (contrib_stats.hip): an entry's per-pixel values are
 * reduced inside the wave that walks the quadrant, then one atomic per statistic per (wave, entry).  weight_max, pixel_count and
 * dominant_count are bit-reproducible -- a maximum and integer sums do not depend on the order --; weight_sum is NOT: float atomics
 * add in the order the waves arrive (each result is the float32 sum of the same terms in some order).  No allocation, no
 * device->host read-back, no host wait.
 * Checks, in this order: the parameters (as every entry); P == 0 -> GSR_OK, nothing written; a NULL geom, binning or image ->
 * GSR_ERR_INVALID; all four outputs NULL -> GSR_ERR_INVALID; then the arena's record -> GSR_ERR_INVALID when V, P, W or H differ from
 * the last forward or recolor on `geom` (the outputs are then untouched; an arena without a record is not checked; the record is read,
 * never written); then the sizes of the three allocations (GSR_ERR_CAPACITY). */
int gsr_contrib_stats(const gsr_params* p, int V, const int* radii /* [V][P], may be NULL */, const void* geom, size_t geom_bytes,
                      const void* binning, size_t binning_bytes, const void* image, size_t image_bytes,
                      const float* pixel_weights /* [V][H][W] or NULL */, int accumulate, float* weight_sum /* [P] or NULL */,
                      float* weight_max /* [P] or NULL */, int* pixel_count /* [P] or NULL */, int* dominant_count /* [P] or NULL */,
                      gsr_stream_t stream);

/* Photometric loss of the rendered frames and its gradient: per view v, loss = (1 - lambda) L1 + lambda (1 - SSIM), the loss nearly
 * every Gaussian-splat trainer uses, evaluated in HIP from the frames exactly as the forwards return them (out_color: [V][3][..][..],
 * planar), so that dL_dimage is what gsr_backward_batch takes as dL_dpix.  W and H are the resolution of the loss, which is the
 * target's; the frames are ss times as large each way.
 *   Definition, per view and channel.  x = image for ss = 1; for ss = 2, x = ((i00 + i01) + (i10 + i11)) * 0.25 over each 2 x 2 block
 * (what a bilinear down-filter with align_corners = false does at rate 2).  y = target.  w = the normalised 11 x 11 Gaussian window,
 * sigma 1.5, separable: g[k] ~ exp(-(k - 5)^2 / 4.5).  conv = correlation with w under zero padding of 5.  mu1 = conv(x), mu2 = conv(y),
 * s1 = conv(x x) - mu1^2, s2 = conv(y y) - mu2^2, s12 = conv(x y) - mu1 mu2, C1 = 1e-4, C2 = 9e-4,
 * m = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)).
 *   loss_terms[v] = { mean |x - y|,  mean m,  mean (x - y)^2,  (1 - lambda) [0] + lambda (1 - [1]) }, means over the 3 H W values of
 * the view; [3] is formed from the float32 values [0] and [1] with one rounding.
 *   dL_dimage = dL_dloss[v] * d loss_terms[v][3] / d image (dL_dloss NULL: 1 for every view): the L1 part is
 * (1 - lambda) sign(x - y) / (3 H W) with sign(0) = 0; the SSIM part is -lambda / (3 H W) (conv(A) + 2 x conv(B) + y conv(C)) with the
 * three maps A = dm/dmu1 - 2 mu1 B - mu2 C, B = dm/ds1, C = dm/ds12 the forward saved; with ss = 2 each of the four source pixels
 * receives a quarter.  Every element of dL_dimage is written.  image == target gives an L1 part and an SSIM part of exactly 0.
 *   state: a caller-owned device block of at least gsr_image_loss_state_bytes(V, W, H) bytes, opaque (the three maps, 36 B per loss
 * pixel, and the workgroups' partial sums).  The size query is a pure host function; its result is a multiple of 256, does not
 * decrease in any argument, and is 0 for sizes the forward refuses.  state = NULL in the forward: metrics only -- loss_terms is
 * written, with the same bits as a call with a state block, by ONE workgroup per view (there is nowhere to keep partial sums: the call
 * is as slow as one compute unit per view; pass a state block where the time matters).  The backward is valid any number of times
 * after a forward with the same V, W, H, ss, lambda, image, target and state; that it follows such a forward is the CALLER'S duty:
 * the library keeps no record of it and cannot refuse a backward on a block some other forward wrote.
 *   Nothing is read back from the device, no host wait is made, nothing is allocated.  No float atomics: every workgroup stores its
 * three sums as float64 into the state block and a second small launch adds a view's partials by index and rounds once, so all
 * outputs are bit-identical from call to call, and view v of a batch is bit-identical to the same view submitted alone.
 *   Refused, in this order, before any device call: V outside 1..256; W or H < 1, or 3 V H W ss^2 >= 2^31 (or more than 2^24
 * tiles x channels per view); ss other than 1 and 2 (GSR_ERR_INVALID: other rates are never approximated -- down-filter first and
 * pass ss = 1); lambda outside 0..1 or NaN; a NULL image, target, loss_terms, dL_dimage, or (backward) state: GSR_ERR_INVALID; a state
 * block that is too small: GSR_ERR_CAPACITY, the message names the size needed. */
size_t gsr_image_loss_state_bytes(int V, int W, int H);
int gsr_image_loss_forward(int V, int W, int H, int ss, float lambda_dssim, const float* image /* [V][3][H ss][W ss] */,
                           const float* target /* [V][3][H][W] */, float* loss_terms /* [V][4] */, void* state /* or NULL */,
                           size_t state_bytes, gsr_stream_t stream);
int gsr_image_loss_backward(int V, int W, int H, int ss, float lambda_dssim, const float* image, const float* target,
                            const float* dL_dloss /* [V] or NULL */, const void* state, size_t state_bytes,
                            float* dL_dimage /* [V][3][H ss][W ss] */, gsr_stream_t stream);

/* The optimizer step of a training iteration: Adam (torch.optim.Adam without amsgrad, weight_decay or maximize) over the 1..8 parameter
 * groups of one cloud in ONE launch, with an optional per-Gaussian visibility mask (the "sparse Adam" of splat trainers: a Gaussian no
 * view of the batch saw keeps its parameters AND its moments, instead of drifting on stale momentum).
 *   gsr_visible_from_radii: visible[i] = any_v(radii[v][i] > 0) for the radii [V][P] a batch forward returned; every element of
 * visible [P] is written (0 or 1).
 *   gsr_adam_step.  A group is four float32 device arrays of P * width elements, row-major [P][width]: param, grad, exp_avg,
 * exp_avg_sq, with its own width >= 1 and learning rate lr; `groups` is a HOST array of G of them, copied into the kernel's arguments.
 * t is the number of this step, 1 for the first.  Definition, per element, in float32 with one rounding per written operation, where
 * b1 = beta1, b2 = beta2 and eps are the float32 values passed:
 *     c1 = 1.0f - b1,  c2 = 1.0f - b2
 *     m' = b1 * m + c1 * g
 *     v' = b2 * v + c2 * (g * g)
 *     p' = p - step_g * (m' / (sqrtf(v') * rsq2 + eps))
 * with the two constants formed on the host in double and rounded once to float32:
 *     step_g = lr_g / (1 - b1^t),   rsq2 = 1 / sqrt(1 - b2^t)
 * param, exp_avg and exp_avg_sq are updated in place.  A non-finite gradient propagates as it does in torch: there is no guard.
 *   visible: uint8 [P] on the device, or NULL.  With a mask, the rows i with visible[i] == 0 are untouched: param, exp_avg and
 * exp_avg_sq keep their bits.  Without a mask every row is updated.
 *   zero_grads != 0: every element of every group's grad is written to 0 after it has been consumed, masked rows included.
 *   Pointers need only the 4-byte alignment of their type: a group whose four arrays are all 16-byte aligned is walked 16 B per lane,
 * any other group, and the last P * width % 4 elements, element by element, with the same bits.
 *   Nothing is read back from the device, no host wait is made, nothing is allocated.  There are no atomics.  Outputs are bit-identical
 * from call to call; a group's result does not depend on which other groups share the call; rows [a, b) submitted alone (offset
 * pointers, P = b - a) get the bits they get in the whole call.
 *   Refused, in this order, before any device call, each with GSR_ERR_INVALID: G outside 1..8; P < 1, a width < 1 or a
 * P * width >= 2^31; t < 1; beta1 or beta2 outside [0, 1) or NaN, eps <= 0 or not finite, an lr negative or not finite; groups NULL or
 * one of a group's four pointers NULL.  gsr_visible_from_radii refuses V outside 1..256, then P < 1 or V * P >= 2^31, then a NULL
 * radii or visible. */
typedef struct {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int width;
    float lr;
} gsr_adam_group;
int gsr_visible_from_radii(int V, int P, const int32_t* radii /* [V][P] */, uint8_t* visible /* [P] */, gsr_stream_t stream);
int gsr_adam_step(int P, int G, const gsr_adam_group* groups /* HOST array */, int64_t t, float beta1, float beta2, float eps,
                  const uint8_t* visible /* [P] or NULL */, int zero_grads, gsr_stream_t stream);

/* Adaptive density control: clone, split and prune in one pass.  The decision of 3DGS's densify_and_prune from the statistics
 * gsr_backward_view_stats leaves, restated so that one pass over the cloud evaluates it (gsr_density_plan), and the new cloud built
 * from the plan (gsr_density_apply).
 *   Decision inputs per Gaussian i: scales[i][3], opacities[i], grad_norm_sum[i] (float32), visible_views[i] and max_radius[i]
 * (int32), and optionally prune_mask[i] (uint8, NULL = none).  The rule (gsr_density_rule, a HOST struct, copied into the kernel's
 * arguments): grad_threshold; dense_size (3DGS: percent_dense x extent); min_opacity, compared in the STORED domain (a caller that
 * stores logits passes logit(0.005)); max_screen_radius (int, 0 = test off); max_world_size (float, 0 = test off; 3DGS: 0.1 x extent);
 * log_scales (0/1); normalize_rotations (0/1); seed.
 *   Derived, in float32 with one rounding per written operation:
 *     sigma = scales             (log_scales = 0)        sigma = expf(scales)   (log_scales = 1)
 *     smax  = max(sigma_x, sigma_y, sigma_z)
 *     g     = grad_norm_sum / (float)max(visible_views, 1)
 * A NaN compares false everywhere, as in torch: a NaN gradient densifies nothing.
 *   Actions, evaluated in this order (the set of rows is what 3DGS produces when clone, split and prune run one after the other):
 *     hot  = g >= grad_threshold
 *     dead = opacities[i] < min_opacity || (prune_mask && prune_mask[i])
 *     big  = (max_screen_radius > 0 && max_radius[i] > max_screen_radius) || (max_world_size > 0 && smax > max_world_size)
 *     hot && smax <= dense_size   clone:  dead -> no rows (GSR_DENSITY_PRUNED); big -> the copy alone, one row marked new
 *                                 (GSR_DENSITY_CLONED_COPY); else the original and a bit-identical copy (GSR_DENSITY_CLONED).  The
 *                                 screen-radius and world-size tests apply to the original only: a copy starts with radius 0
 *     hot && smax >  dense_size   split:  dead || (max_world_size > 0 && smax / 1.6f > max_world_size) -> no rows
 *                                 (GSR_DENSITY_PRUNED); else the parent is removed and two children are made (GSR_DENSITY_SPLIT).
 *                                 The screen-radius test does not apply to children
 *     otherwise                   dead || big -> no rows (GSR_DENSITY_PRUNED); else one row (GSR_DENSITY_KEPT)
 * so every Gaussian yields c_i in {0, 1, 2} output rows.
 *   Output order: ascending source index, a Gaussian's rows adjacent, the original before its copy and child 0 before child 1 (not
 * 3DGS's "kept, then clones, then children": this one is an exclusive scan of c_i and keeps a spatially ordered cloud ordered).
 *   gsr_density_plan writes offsets [P + 1], the exclusive prefix of c_i with offsets[P] = P'; action [P], the GSR_DENSITY_* code of
 * every Gaussian; and totals [5] (int64, DEVICE) = {P', carried rows (kept Gaussians and the originals of clones), copies made,
 * children made, source Gaussians that left no row}.  Three launches: decide and count per workgroup, a scan of the workgroup counts
 * by one workgroup (looped: any P up to the limit), the final offsets.  scratch holds the workgroup counts:
 * gsr_density_scratch_bytes(P) bytes, a pure host function, a multiple of 256, 0 for a refused P.
 *   gsr_density_apply builds the output rows of 1..8 groups from the plan, which it only reads: it may be called several times with
 * different group tables (parameters, then exp_avg, then exp_avg_sq).  A group is a float32 source [P][width], a destination
 * [P_out][width] and a role (`groups` is a HOST array, copied into the kernel's arguments); src and dst must not overlap:
 *     GSR_DENSITY_COPY     every row takes its source row's bits
 *     GSR_DENSITY_MEANS    width 3; a child is displaced (below), every other row takes its source row's bits
 *     GSR_DENSITY_SCALES   width 3; a child's scales are sigma' = sigma / 1.6f (log_scales = 0: one float32 division) or
 *                          s' = s - 0x1.e148a2p-2f (log_scales = 1: the float32 nearest log(1.6), one subtraction)
 *     GSR_DENSITY_MOMENT   a carried row (kept, or the original of a clone) takes its source row's bits, a new row (copy or child) +0
 * index (int32 [P_out], or NULL) receives i for a carried row and -1 - i for a new row made from parent i: negative means "zero
 * moments" to a re-indexing optimizer, and still names the parent.  P_out is the caller's copy of offsets[P]; every store is bounded
 * by it, so a stale value can truncate the output but never write past dst.  P_out = 0: GSR_OK, nothing is written.
 *   Child mean.  Child k in {0, 1} of parent i: with (r, x, y, z) the stored quaternion -- as it is (normalize_rotations = 0: what
 * the rasterizer renders) or each component divided by n = sqrtf(((r r + x x) + y y) + z z) (normalize_rotations = 1) -- and R the
 * rotation the rasterizer builds from it,
 *     R[0] = (1 - 2 (y y + z z),  2 (x y - r z),      2 (x z + r y))
 *     R[1] = (2 (x y + r z),      1 - 2 (x x + z z),  2 (y z - r x))
 *     R[2] = (2 (x z - r y),      2 (y z + r x),      1 - 2 (x x + y y))
 *     t = sigma * eps (componentwise);   d_r = (R[r][0] t0 + R[r][1] t1) + R[r][2] t2;   mu'_r = mu_r + d_r
 * in float32, one rounding per written operation.  Every other value of a child or a copy is the parent's bits.
 *   Noise eps: the caller's noise (float32 [P][2][3], indexed by source and child, read for splits only), or with noise = NULL a
 * counter-based generator: Philox4x32-10 with the multipliers 0xD2511F53 (on word 0) and 0xCD9E8D57 (on word 2), the key increments
 * 0x9E3779B9 and 0xBB67AE85 (the key is bumped between rounds, nine times), key = (low half of seed, high half of seed), counter =
 * (i, k, 0, 0); a round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).  The four output
 * words x_j give, in float32,
 *     u_j = ((float)(x_j >> 8) + 0.5f) * 0x1p-24f          (the sum rounds to even from x_j >> 8 = 2^23 on: u_j lies in (0, 1])
 *     r01 = sqrtf(-2.0f * logf(u0));   eps0 = r01 * cosf(6.2831855f * u1);   eps1 = r01 * sinf(6.2831855f * u1)
 *     eps2 = sqrtf(-2.0f * logf(u2)) * cosf(6.2831855f * u3)
 * so eps depends on (seed, i, k) alone: not on P, the launch shape or other Gaussians.  Sub-ranges: rows [a, b) planned and applied
 * alone (offset pointers, P = b - a, caller noise offset likewise) get the bits they get in the whole call; with noise = NULL the
 * counter is the CALL's i, so a sub-range draws other noise than the whole.
 *   Nothing is read back from the device, no host wait is made, nothing is allocated.  There are no atomics.  Outputs are
 * bit-identical from call to call; a group's result does not depend on which other groups share the call.  Groups whose src and dst
 * are 16-byte aligned and whose width is a multiple of 4 move 16 B per lane, every other group element by element, with the same bits.
 *   Refused, in this order, before any device call, with GSR_ERR_INVALID unless noted: P < 1 or 2 P >= 2^31; (apply) G outside 1..8, a
 * width < 1 or 2 P width >= 2^31, a role that is none of the four; (apply) a MEANS or SCALES group whose width is not 3; (apply) more
 * than one MEANS or more than one SCALES group; a rule with a negative or non-finite grad_threshold, dense_size or max_world_size, a
 * negative max_screen_radius or a NaN min_opacity; a NULL required pointer (plan: rule, scales, opacities, grad_norm_sum,
 * visible_views, max_radius, offsets, action, totals, scratch; apply: groups, rule, a group's src or dst, offsets, action, and scales
 * and rotations when a MEANS group is present); (apply) P_out negative or above 2 P; (plan) scratch smaller than
 * gsr_density_scratch_bytes(P): GSR_ERR_CAPACITY, the message names the size needed. */
#define GSR_DENSITY_PRUNED 0      /* no row */
#define GSR_DENSITY_KEPT 1        /* one row, carried */
#define GSR_DENSITY_CLONED 2      /* two rows: the original (carried) and its copy (new) */
#define GSR_DENSITY_CLONED_COPY 3 /* one row: the copy (new); the original failed the screen-radius or world-size test */
#define GSR_DENSITY_SPLIT 4       /* two rows: the children (new) */
#define GSR_DENSITY_COPY 0
#define GSR_DENSITY_MEANS 1
#define GSR_DENSITY_SCALES 2
#define GSR_DENSITY_MOMENT 3
typedef struct {
    float grad_threshold;
    float dense_size;
    float min_opacity;
    int max_screen_radius;
    float max_world_size;
    int log_scales;
    int normalize_rotations;
    uint64_t seed;
} gsr_density_rule;
typedef struct {
    const float* src;
    float* dst;
    int width;
    int role;
} gsr_density_group;
size_t gsr_density_scratch_bytes(int P);
int gsr_density_plan(int P, const gsr_density_rule* rule, const float* scales /* [P][3] */, const float* opacities /* [P] */,
                     const float* grad_norm_sum /* [P] */, const int32_t* visible_views /* [P] */, const int32_t* max_radius /* [P] */,
                     const uint8_t* prune_mask /* [P] or NULL */, uint32_t* offsets /* [P + 1] */, uint8_t* action /* [P] */,
                     int64_t* totals /* [5], DEVICE */, void* scratch, size_t scratch_bytes, gsr_stream_t stream);
int gsr_density_apply(int P, int G, const gsr_density_group* groups /* HOST array */, const gsr_density_rule* rule,
                      const uint32_t* offsets /* [P + 1] */, const uint8_t* action /* [P] */, const float* scales /* [P][3] or NULL */,
                      const float* rotations /* [P][4] or NULL */, const float* noise /* [P][2][3] or NULL */,
                      int32_t* index /* [P_out] or NULL */, int64_t P_out, gsr_stream_t stream);

/* Point-cloud neighbourhoods: exact k nearest neighbours, spacing, PCA normals and orientations (cloud_geometry.hip).  What a raw
 * point cloud needs to become Gaussians: the mean nearest-neighbour distance that sets the scale (3DGS's distCUDA2 with k_s = 3), a
 * normal per point, and the frame of an oriented disc.
 *   gsr_knn.  points is float32 [P][3] on the device.  A point with a non-finite coordinate is absent: it is nobody's neighbour and
 * its own row is all padding.  For present points i and j, in float32 with one rounding per written operation,
 *     dx = x_i - x_j;  dy = y_i - y_j;  dz = z_i - z_j;      d2(i, j) = (dx dx + dy dy) + dz dz
 * Row i of the result holds the K present points j != i with the smallest (d2, j) in lexicographic order -- ties go to the lower
 * index --, ascending, in idx [P][K] (int32) and d2 [P][K] (float32, or NULL: not wanted).  Slots beyond the available neighbours hold
 * idx = -1 and d2 = +inf; a neighbour whose d2 overflowed to +inf still precedes the padding.  Coincident points are each other's
 * neighbours at d2 = 0.  The result is a function of the input alone: the search is exact, its traversal order cannot show, and two
 * calls give the same bits.  K in 1..32, 1 <= P < 2^30.
 *   How: the bounding box of the present points from a two-stage min/max reduction (it stays on the device), a 30-bit Morton key per
 * point (absent points keyed last), the library's radix sort, a tight box around every run of 64 sorted points and around every 64
 * such runs, and one wave per run that answers its 64 queries: it walks its own run, the runs of its own coarse box, then the other
 * coarse boxes and the runs inside those that survive.  A box is skipped only when, for every lane, the float32 bound
 *     g_a = max(lo_a - q_a, q_a - hi_a, 0)   per axis a;      bound = (g_x g_x + g_y g_y) + g_z g_z
 * is strictly greater than the lane's current K-th distance: rounding is monotone, so the bound is <= d2 of every point inside the
 * box, and on equality a lower index may still be inside.  Every box is walked at most once per run, whatever the cloud.
 *   scratch: gsr_knn_scratch_bytes(P, K) bytes from the caller (a pure host function, a multiple of 256, monotone in P and K, 0 for a
 * refused P or K); its contents on entry do not matter.  Nothing is read back from the device, no host wait is made, nothing is
 * allocated.  There are no atomics.
 *   Refused before any device call, in this order: P < 1 or P >= 2^30 or K outside 1..32 (GSR_ERR_INVALID); points, idx or scratch
 * NULL (GSR_ERR_INVALID); scratch_bytes < gsr_knn_scratch_bytes(P, K) (GSR_ERR_CAPACITY, the message names the size needed).
 *
 *   gsr_cloud_geometry.  One lane per point, no scratch.  knn_idx is [P][K] as gsr_knn writes it; any int32 is allowed in it.  Entry j
 * of row i is PRESENT when 0 <= j < P and point j has three finite coordinates; a point i that has a non-finite coordinate has no
 * present entry.  Every other entry (-1, out of range) contributes nothing.  With delta_j = p_j - p_i (componentwise, float32):
 *   spacing [P]: over the first n_s = min(k_s, present) present entries in list order, sum = sum + ((dx dx + dy dy) + dz dz) starting
 * from 0;  spacing = sqrtf(sum / (float)n_s), and 0 when n_s = 0.  With k_s = 3 this is 3DGS's initial scale.
 *   cov6 [P][6]: the neighbourhood is the point itself (delta = 0) and its first n_n = min(k_n, present) present entries, n = n_n + 1
 * samples.  s = sum of delta_j in list order starting from 0;  m = s / (float)n;  with e_j = delta_j - m and e_self = 0 - m,
 *     acc_ab = e_self_a e_self_b, then acc_ab = acc_ab + e_j_a e_j_b in list order;      C_ab = acc_ab / (float)n
 * stored as (C_xx, C_xy, C_xz, C_yy, C_yz, C_zz).  n_n < 2 is a DEGENERATE ROW: cov6 = 0, eigenvalues = 0, normal (0, 0, 1), rotation
 * (1, 0, 0, 0); its spacing is still the formula above.  No output of a degenerate row is NaN.
 *   eigenvalues [P][3], ascending: cyclic Jacobi on A = C with V = I, GSR_CLOUD_JACOBI_SWEEPS sweeps over the pairs (p, q) = (0, 1),
 * (0, 2), (1, 2), r the third index.  A pair with A_pq == 0 is left alone; otherwise
 *     theta = (A_qq - A_pp) / (2 A_pq);   t = sgn / (|theta| + sqrtf(theta theta + 1)), sgn = 1 for theta >= 0 else -1
 *     c = 1 / sqrtf(t t + 1);   s = t c;   h = t A_pq
 *     A_pp = A_pp - h;   A_qq = A_qq + h;   A_pq = 0;   (A_rp, A_rq) = (c A_rp - s A_rq, s A_rp + c A_rq)
 *     (V_kp, V_kq) = (c V_kp - s V_kq, s V_kp + c V_kq) for k = 0, 1, 2
 * using only + - x / sqrtf: no closed-form trigonometric solver.  The diagonal and the columns of V are then ordered by three
 * compare-exchanges on the positions (0, 1), (1, 2), (0, 1), each a swap when the left value is greater.
 *   normals [P][3]: u = column 0 of the ordered V;  n = u / sqrtf((u_x u_x + u_y u_y) + u_z u_z).  Sign: with orient_to (HOST
 * float[3], copied into the kernel's arguments) n is negated when (n_x (x_i - o_x) + n_y (y_i - o_y)) + n_z (z_i - o_z) < 0, so that
 * n . (p - orient_to) >= 0; without it n is negated when its first non-zero component is negative.
 *   rotations [P][4], a unit quaternion (r, x, y, z) with r >= 0 in the convention of the density-control section above: its rotation
 * matrix has the columns (a, b, n) with a = column 2 of the ordered V normalised like n, and b = n x a = (n_y a_z - n_z a_y,
 * n_z a_x - n_x a_z, n_x a_y - n_y a_x).  With R_i0 = a_i, R_i1 = b_i, R_i2 = n_i and tr = (R_00 + R_11) + R_22:
 *     tr > 0:                      w = sqrtf(tr + 1) 2;            (r, x, y, z) = (w / 4, (R_21 - R_12) / w, (R_02 - R_20) / w, (R_10 - R_01) / w)
 *     else R_00 > R_11, R_00 > R_22: w = sqrtf(((1 + R_00) - R_11) - R_22) 2;  ((R_21 - R_12) / w, w / 4, (R_01 + R_10) / w, (R_02 + R_20) / w)
 *     else R_11 > R_22:            w = sqrtf(((1 + R_11) - R_00) - R_22) 2;  ((R_02 - R_20) / w, (R_01 + R_10) / w, w / 4, (R_12 + R_21) / w)
 *     else                         w = sqrtf(((1 + R_22) - R_00) - R_11) 2;  ((R_10 - R_01) / w, (R_02 + R_20) / w, (R_12 + R_21) / w, w / 4)
 * then every component is divided by sqrtf(((r r + x x) + y y) + z z), and all four are negated when r < 0.  The matching scales of an
 * oriented Gaussian are sqrt of (lambda_2, lambda_1, lambda_0).
 *   Every output pointer is optional (NULL: not wanted); an output's bits do not depend on which others are asked for.  Nothing is
 * read back, no host wait is made, nothing is allocated, there are no atomics, and two calls give the same bits.
 *   Refused before any device call, in this order, with GSR_ERR_INVALID: P < 1 or P >= 2^30, K outside 1..32, k_s or k_n outside
 * 1..K; points or knn_idx NULL; every output NULL. */
#define GSR_CLOUD_JACOBI_SWEEPS 5
size_t gsr_knn_scratch_bytes(int P, int K);
int gsr_knn(int P, const float* points /* [P][3] */, int K, int32_t* idx /* [P][K] */, float* d2 /* [P][K] or NULL */, void* scratch,
            size_t scratch_bytes, gsr_stream_t stream);
int gsr_cloud_geometry(int P, const float* points /* [P][3] */, int K, const int32_t* knn_idx /* [P][K] */, int k_s, int k_n,
                       const float* orient_to /* HOST [3] or NULL */, float* spacing /* [P] or NULL */, float* cov6 /* [P][6] or NULL */,
                       float* eigenvalues /* [P][3] or NULL */, float* normals /* [P][3] or NULL */, float* rotations /* [P][4] or NULL */,
                       gsr_stream_t stream);

/* Pairs in the lists of the calling thread's last forward call, per view (out[V], HOST array): what a binning arena has to
 * hold.  Equal to num_rendered with reference_lists = 1. */
int gsr_last_list_pairs(int64_t* out, int V);

/* present[i] = (view-space z of means3D[i] > 0.2)   (rasterizer_impl.cu:54-66) */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, gsr_stream_t stream);

/* Inspection of the private arenas (view 0 of a batch; pass a view's sub-arena pointers for the others), for parity tests
 * and the roofline report only (device->device copies into caller buffers; not part of the hot path).  `what` is one of
 * GSR_Q_*. */
#define GSR_Q_DEPTHS 1         /* float  [P]    view-space z of visible Gaussians (0 otherwise)            */
#define GSR_Q_MEANS2D 2        /* float  [P,2]                                                              */
#define GSR_Q_CONIC_OPACITY 3  /* float  [P,4]                                                              */
#define GSR_Q_RGB 4            /* float  [P,3]                                                              */
#define GSR_Q_TILES_TOUCHED 5  /* uint32 [P]                                                                */
#define GSR_Q_POINT_LIST 6     /* uint32 [L]   Gaussian ids sorted by (tile, depth bits, id); L = GSR_Q_LIST_PAIRS[0] (pass it as R) */
#define GSR_Q_POINT_LIST_KEYS 7/* uint64 [L]   (tile<<32)|depth bits, rebuilt for comparison with CUB keys  */
#define GSR_Q_RANGES 8         /* uint32 [T,2]                                                              */
#define GSR_Q_FINAL_T 9        /* float  [H*W]                                                              */
#define GSR_Q_N_CONTRIB 10     /* uint32 [H*W]                                                              */
#define GSR_Q_TILE_NEED 12     /* uint32 [T]   list entries the tile's render actually walked (roofline model)    */
#define GSR_Q_CLAMPED 11       /* uint8  [P,3]                                                              */
#define GSR_Q_LIST_PAIRS 14    /* uint64 [2]   pairs in the view's lists, pairs of the reference's rectangles      */
#define GSR_Q_DEPTH_SORT 13    /* uint32 [4]   depth sort of the frame: key base, key bits compared, passes run, -  */
int gsr_query(const gsr_params* p, int what, const void* geom, const void* binning, size_t binning_bytes, const void* image,
              int64_t num_rendered, void* dst, size_t dst_bytes, gsr_stream_t stream);

/* Per-stage timing of the calls made since gsr_set_profiling(1) (ms, hipEvents on each call's launch stream; the switch is
 * process wide, the records are kept per stream and returned stream by stream).  names/ms hold up to `cap` entries;
 * returns the count and resets the records.  gsr_set_profiling(2) times only the two render kernels (one event pair per
 * forward and per backward: cheap enough to leave on inside a timed region); 0 switches it off. */
void gsr_set_profiling(int on);
int gsr_get_profile(const char** names, float* ms, int cap);

/* Shader-clock probe (bench / profiles only): enqueues a one-wave kernel on `stream` that spins through `iters` x 64 dependent FMAs
 * (about iters x 0.15 us) and stores two 64-bit counts at dst16 (device memory, 16 bytes): elapsed shader-clock ticks (s_memtime) and
 * elapsed ticks of the constant-rate wall clock (s_memrealtime, gsr_wall_clock_khz() ticks per millisecond).  Their ratio x the wall
 * rate is the shader clock the device sustained while the probe was resident -- launched on a side stream it reads the clock UNDER
 * the load of the kernels running beside it.  Nothing in the library waits for it. */
int gsr_clock_probe_launch(void* dst16, int iters, gsr_stream_t stream);
int gsr_wall_clock_khz(void);

/* Device self-test of internal primitives (the matrix-core pixel contraction of the render backward, the ordered reduction of the
 * deterministic backward and that of the extra channels against host sums in the same order, stable radix sort vs std::stable_sort).
 * Allocates its own small buffers; not part of the hot path.  0 = pass. */
int gsr_selftest(gsr_stream_t stream);

/* Test probes of the pair-list machinery (tests only; they allocate, synchronise and are not part of the hot path).
 *
 * gsr_sort_probe runs the library's stable radix sort on bits [0, end_bit) of V independent problems of DEVICE arrays: view v's keys
 * (uint32_t, or uint16_t with GSR_SORT_KEY16), values and outputs start v * stride bytes behind the view-0 pointers.  vals NULL: the
 * value of element i is i.  n_dev NULL: every view holds cap elements; else view v holds min(*(n_dev + v * n_stride bytes), cap).
 * The inputs are copied into work buffers of the call and never modified.  keys_out / vals_out receive cap elements per view from
 * the ping-pong buffer the sort's own rule names; only the first min(count, cap) mean anything.  Key bits at and above end_bit do
 * not take part in the order and come back intact.
 * GSR_SORT_SMALL_BLOCKS: the half-size sort blocks (uint32_t keys, end_bit a multiple of 8).  GSR_SORT_DEPTH_CTL: the depth sort's
 * control words (32 bits of uint32_t keys, index values): keys equal to 0xFFFFFFFF are culled entries whose place is immaterial, the
 * passes above the visible keys' span are skipped, and ctl_out (device, uint32 [V][4]) receives per view: key base, key bits compared,
 * passes run, 0 -- view v's result is read from buffer (passes run & 1).  A combination the sort has no kernel for is refused with
 * GSR_ERR_INVALID before any device call, never replaced by another kernel.  cap == 0: OK, nothing is touched. */
#define GSR_SORT_KEY16 1
#define GSR_SORT_SMALL_BLOCKS 2
#define GSR_SORT_DEPTH_CTL 4
int gsr_sort_probe(const void* keys, const uint32_t* vals, size_t stride, const uint64_t* n_dev, size_t n_stride, int V, int64_t cap,
                   int end_bit, int flags, void* keys_out, uint32_t* vals_out, uint32_t* ctl_out, gsr_stream_t stream);

/* gsr_tile_ranges_probe runs the tile-range search on V views of sorted DEVICE keys (tile ids < T; uint16_t when key16): view v has
 * min(*(n_dev + v * n_stride bytes), cap) keys at keys + v * stride bytes.  ranges (device, uint32 [V][T][2]) receives (first, one
 * past last) list position per tile, (0, 0) for a tile without keys.  Every tile is written.  The call waits for the kernel. */
int gsr_tile_ranges_probe(const void* keys, size_t stride, const uint64_t* n_dev, size_t n_stride, int V, int64_t cap, int T, int key16,
                          uint32_t* ranges, gsr_stream_t stream);

/* Number of device->host read-backs the library has made in this process: exactly one per forward call -- the 32-byte
 * per-view counter block (num_rendered, trap and stall flags), which the pair-emission kernel stores into mapped host
 * memory and the host reads after ONE event wait, once the whole frame is enqueued -- and none per backward.  There is no
 * copy command in the stream.  For tests that guard the call path against host stalls. */
long long gsr_d2h_count(void);

/* Tuning / test hook: submissions of up to `views` views run the forward render in half-quadrant mode (csrc/render_fwd.hip: a wave
 * owns 8 x 4 pixels twice and blends four list entries per step -- a shorter critical path for the deep walks a single view's launch
 * ends on; images, final_T and n_contrib are bit-identical in both modes).  Default 1 (GSR_FWD_HALF_V in the environment), 0 = the
 * 8 x 8 kernel always; views < 0 only queries.  Returns the value in force. */
int gsr_set_forward_half_views(int views);

/* Accuracy / speed switch of the render backward's pixel contraction (GSR_BWD_SUBQ in the environment): 0 second moments about the
 * 8 x 8 quadrant centre, shifted to the splat centre per entry: the mean2D / conic sums carry 1.85x / 4.3x the reference build's own
 * rounding error (median over 500 fuzz cases against a float64 evaluation of the same sums; two orders of magnitude inside every
 * test bar); 1 about the centres of the four 4 x 4 sub-quadrants, each shifted on its own: 1.25x / 2.0x, +8 % kernel time;
 * 2 (DEFAULT) adaptive: the sub-quadrant path only for batches of eight entries that hold a splat more than sqrt(20) of its own sigmas
 * from the quadrant centre -- where that rounding comes from (sub-pixel splats seen from a quadrant away): 1.33x / 2.1x at +0.8 %
 * kernel time on the benchmark views, none of whose batches takes it (profiles/r06_bwd_accuracy.txt).  mode < 0 only queries.
 * Returns the value in force. */
int gsr_set_backward_moments(int mode);

/* Arithmetic of the forward render of INFERENCE calls (GSR_RENDER_MATH in the environment, read when the library is first used):
 * 0 (DEFAULT) exact: the reference's operations one rounding at a time; images, final_T and n_contrib equal a strict-order build of
 * the reference bit for bit.  1 fast (csrc/render_math.hpp): the constants -0.5 log2(e) / -log2(e) folded into the conic once per staged
 * entry, the power as two multiplies and two fused multiply-adds, alpha = min(0.99, o 2^p) on the hardware's exp2 without range
 * reduction, and one fused multiply-add per blended channel.  What the fast mode promises: it is deterministic from call to call (and
 * the same in both forward kernels, alone or in a batch); radii, num_rendered, lists and ranges are those of the exact mode; every
 * alpha is as accurate against float64 as the exact mode's, so images lie within the contract's 1e-4 of the exact mode's except at
 * pixels where an alpha sits on the 1/255 cut or a transmittance on the 1e-4 stop and the decision falls the other way (the reference
 * as shipped, compiled with FMA contraction, differs from its strict build in the same way).  What it does not promise: bit-identity
 * with any build of the reference.  The mode is a permission, not a demand: it applies to forwards that save nothing for a backward
 * (need_backward = 0: gsr_forward_batch, gsr_forward_batch_channels, gsr_forward_batch_channels_train, gsr_forward_stage2,
 * gsr_forward_recolor); a forward with need_backward = 1 does not look at this switch (its arithmetic is gsr_set_train_math's, exact
 * by default), and no backward does.  mode < 0 only queries; a value above 1 is refused and changes nothing.  Returns the value in
 * force. */
int gsr_set_render_math(int mode);

/* Arithmetic of TRAINING calls: the colour forwards that save for a backward, and the render backward that follows them
 * (GSR_TRAIN_MATH in the environment, read when the library is first used).  0 (DEFAULT) exact, 1 fast; the calling convention is
 * gsr_set_render_math's (mode < 0 only queries; a value above 1 is refused and changes nothing; returns the value in force).  The two
 * switches are independent: neither setter changes the other's value, and a call looks at exactly one of them.
 *   Forwards.  With need_backward = 1, gsr_forward_batch (both forward kernels), gsr_forward_stage2 and gsr_forward_recolor run the
 * fast kernels of gsr_set_render_math(1) -- the same images, final_T and n_contrib bit for bit as an inference call in that mode --
 * and write the saves (slice-boundary states, accumulated colour) from them.  With need_backward = 0 only gsr_set_render_math counts.
 * gsr_forward_batch_channels_train with need_backward = 1 stays exact under both switches: the channels backward has no fast variant
 * (gsr_backward_batch_channels and gsr_backward_batch_channels_det are untouched).
 *   Backwards.  gsr_backward_batch, gsr_backward and gsr_backward_batch_det follow the FORWARD, not the switch: the library's record
 * of the geometry arena holds the arithmetic of the call that last wrote the saves (the forward, or a need_backward recolor, which
 * rewrites all of them), and the render backward re-evaluates p2, G = 2^p2, alpha and the three-part hit test with that forward's own
 * functions, so its decisions are the ones that wrote n_contrib, whatever the switch says at backward time.  An arena without a
 * record (the table is dropped once it holds more than 4096 arenas) takes the switch in force at the backward: keep it where the
 * forward had it.
 *   What the fast mode promises: it is deterministic with itself (gsr_backward_batch_det stays bit-identical from call to call);
 * radii, num_rendered, lists and ranges are the exact mode's; images lie within the contract's 1e-4 of the exact mode's except at
 * threshold decisions (see gsr_set_render_math); gradients are those of the image it rendered, as accurate against a float64
 * evaluation of the same sums as the exact mode's (profiles/r15_train_math.txt).  What it does not promise: bit-identity with any
 * build of the reference, and anything for the channels backward. */
int gsr_set_train_math(int mode);

const char* gsr_last_error(void);
const char* gsr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H */
