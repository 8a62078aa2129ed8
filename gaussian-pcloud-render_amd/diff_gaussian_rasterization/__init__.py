"""diff_gaussian_rasterization -- MI355X-native drop-in for the reference package of the same name.

Public surface mirrors /root/reference/diff-gaussian-rasterization/diff_gaussian_rasterization/__init__.py
field-for-field so the reference's callers (simple_raw_render.py:12,98-111,263-277) run unchanged on
PyTorch-ROCm:

    GaussianRasterizationSettings   NamedTuple, 12 fields, same order        (__init__.py:157-169)
    GaussianRasterizer(nn.Module)   .forward(means3D, means2D, opacities, shs=, colors_precomp=, scales=,
                                    rotations=, cov3D_precomp=) -> (color[3,H,W], radii[P]); .markVisible
                                                                                                (:171-220)
    rasterize_gaussians, _RasterizeGaussians (autograd Function, 9 inputs, grads in input order) (:21-155)
    cpu_deep_copy_tuple                                                                         (:17-19)

Underneath, ``_native`` (ctypes over the C-ABI HIP library, include/gsr.h) takes the place of the pybind
module ``_C``.  No CPU path exists: tensors must live on a HIP device.
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _native as _C
from ._native import get_deterministic, set_deterministic  # noqa: F401  (the deterministic-backward switch)
from ._native import get_deterministic_channels, set_deterministic_channels  # noqa: F401  (the deterministic channels backward's own switch)
from ._native import get_render_math, set_render_math  # noqa: F401  (arithmetic mode of the inference forwards)
from ._native import get_train_math, set_train_math  # noqa: F401  (arithmetic mode of the training forwards and their backward)


def cpu_deep_copy_tuple(input_tuple):
    """Host copies of every tensor of an argument tuple (what the debug snapshots store); other items pass through."""
    return tuple(x.cpu().clone() if isinstance(x, torch.Tensor) else x for x in input_tuple)


def _native_call(fn, args, debug, dump, message, **kw):
    """One call into the native library.  With `debug` the arguments are copied to the host first, and if the call raises they are
    written to `dump` with the reference's message before the exception travels on (reference __init__.py:83-90,132-139)."""
    if not debug:
        return fn(*args, **kw)
    snapshot = cpu_deep_copy_tuple(args)
    try:
        return fn(*args, **kw)
    except Exception:
        torch.save(snapshot, dump)
        print(message)
        raise


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings)


def _or_none(grad, inp):
    """an absent optional was passed as an empty tensor: its gradient slot gets None, not a [P, ...] tensor of the wrong shape
    (autograd validates shapes on ROCm torch 2.x)"""
    return grad if inp.numel() != 0 else None


def _input_grads(grads, ctx, sh, colors_precomp, scales, rotations, cov3Ds_precomp, *rest):
    """The native backward's 8-tuple as the gradients of (means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
    cov3Ds_precomp), the order of forward's inputs, followed by `rest` (the settings get None)."""
    g_means2D, g_colors, g_opacities, g_means3D, g_cov3D, g_sh, g_scales, g_rotations = grads
    return (g_means3D, g_means2D, _or_none(g_sh, sh), _or_none(g_colors, colors_precomp), g_opacities.reshape(ctx.opacity_shape),
            _or_none(g_scales, scales), _or_none(g_rotations, rotations), _or_none(g_cov3D, cov3Ds_precomp)) + rest


_ABSENT = torch.Tensor([])


def _check_sources(shs, colors_precomp, scales, rotations, cov3D_precomp):
    """exactly one colour source and exactly one covariance source (reference __init__.py:190-195: the same exception texts)"""
    if (shs is None) == (colors_precomp is None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    pair_given, pair_complete = scales is not None or rotations is not None, scales is not None and rotations is not None
    if (cov3D_precomp is None and not pair_complete) or (cov3D_precomp is not None and pair_given):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')


def _absent_as_empty(*optionals):
    """absent optionals travel as empty CPU tensors, like the reference's torch.Tensor([]) (:197-206); one shared empty tensor
    instead of a fresh one per call (GaussianRasterizer.forward runs while the GPU waits for the call's first kernel)"""
    return [_ABSENT if t is None else t for t in optionals]


class _RasterizeGaussians(torch.autograd.Function):
    """The per-view call: 9 inputs in the reference's order, (color, radii) out, gradients back in input order (reference
    __init__.py:44-155)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        rs = raster_settings
        if not rs.debug:
            # steady state of a per-view loop: the short path (_native.forward_view; None = take the general one below)
            need_backward = any(ctx.needs_input_grad)
            fast = _C.forward_view(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, need_backward)
            if fast is not None:
                num_rendered, color, radii, arenas, layout = fast
                ctx.raster_settings, ctx.num_rendered, ctx.opacity_shape, ctx.layout = rs, num_rendered, tuple(opacities.shape), layout
                ctx.det_pairs = _C.last_list_pairs(1) if need_backward and _C.deterministic_active() else None
                if need_backward:
                    ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, arenas)
                ctx.mark_non_differentiable(radii)
                return color, radii
        ctx.layout = None
        # the native call's argument order = reference __init__.py:60-80
        args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh, rs.sh_degree, rs.campos, rs.prefiltered,
                rs.debug)
        num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _native_call(
            _C.rasterize_gaussians, args, rs.debug, "snapshot_fw.dump",
            "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.", need_backward=any(ctx.needs_input_grad))
        ctx.raster_settings, ctx.num_rendered, ctx.opacity_shape = rs, num_rendered, tuple(opacities.shape)
        ctx.det_pairs = _C.last_list_pairs(1) if means3D.shape[0] != 0 and _C.deterministic_active() else None
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
                              imgBuffer)
        ctx.mark_non_differentiable(radii)
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _):
        rs = ctx.raster_settings
        if ctx.layout is not None:
            colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, arenas = ctx.saved_tensors
            grads = _C.backward_view(rs, means3D, radii, colors_precomp, scales, rotations, cov3Ds_precomp, grad_out_color, sh, arenas,
                                     ctx.layout, deterministic=_C.deterministic_active(), pairs=ctx.det_pairs)
            return _input_grads(grads, ctx, sh, colors_precomp, scales, rotations, cov3Ds_precomp, None)
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
         imgBuffer) = ctx.saved_tensors
        # the native call's argument order = reference __init__.py:109-129
        args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, sh, rs.sh_degree, rs.campos, geomBuffer, ctx.num_rendered,
                binningBuffer, imgBuffer, rs.debug)
        grads = _native_call(
            _C.rasterize_gaussians_backward, args, rs.debug, "snapshot_bw.dump",
            "\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n", deterministic=_C.deterministic_active(),
            pairs=ctx.det_pairs)
        return _input_grads(grads, ctx, sh, colors_precomp, scales, rotations, cov3Ds_precomp, None)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class GaussianRasterizer(nn.Module):
    """nn.Module like the reference's (no parameters, no buffers: the settings are its only state).  The reference's caller builds one
    PER CALL (simple_raw_render.py:263), between the copies that drain the stream and the first kernel, so construction and call are
    kept off nn.Module's bookkeeping until something asks for it: nn.Module.__init__ (a dozen dictionaries) runs on the first access
    to module state -- hooks, .to(), state_dict(), children ... -- and a module nobody has touched that way is called straight
    through to forward (there can be no hooks on it)."""

    def __init__(self, raster_settings):
        object.__setattr__(self, "raster_settings", raster_settings)

    def __getattr__(self, name):
        if "_parameters" not in self.__dict__:          # nn.Module state asked for: build it now
            rs = self.__dict__.pop("raster_settings")
            nn.Module.__init__(self)
            object.__setattr__(self, "raster_settings", rs)
            return getattr(self, name)
        return nn.Module.__getattr__(self, name)

    def __setattr__(self, name, value):
        if "_parameters" not in self.__dict__:
            self.__getattr__("_parameters")
        nn.Module.__setattr__(self, name, value)

    def __call__(self, *args, **kwargs):
        if "_parameters" not in self.__dict__:
            return self.forward(*args, **kwargs)
        return nn.Module.__call__(self, *args, **kwargs)

    def markVisible(self, positions):
        with torch.no_grad():
            raster_settings = self.raster_settings
            visible = _C.mark_visible(positions, raster_settings.viewmatrix, raster_settings.projmatrix)
        return visible

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        _check_sources(shs, colors_precomp, scales, rotations, cov3D_precomp)
        shs, colors_precomp, scales, rotations, cov3D_precomp = _absent_as_empty(shs, colors_precomp, scales, rotations, cov3D_precomp)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings)


# ---- extension: all views of one cloud in ONE submission ----------------------------------------------------
# The reference's caller loops views in Python, one GaussianRasterizer call each (simple_raw_render.py:259-278).  The entry
# points below take the list of per-view settings instead and hand the whole batch to the C ABI's gsr_forward_batch /
# gsr_backward_batch: one preprocess grid over V x P, one render grid over all views' tiles, and gradients summed over the
# views on the device -- the same numbers as V separate calls whose gradients autograd adds up.
# The per-view matrices of a settings list are packed ONCE into [V,4,4] / [V,4,4] / [V,3] device blocks and remembered:
# a training loop hands over the same settings objects every iteration, and rebuilding the blocks (36 tiny copies + 3 stacks)
# or comparing backgrounds through host memory (a blocking device->host copy per view, which drains the stream) would put
# the host back on the critical path of every call.  Steady state: no torch kernel, no copy, no synchronisation.
#
# What the cache can and cannot see.  A tensor is identified by (address, shape, strides, version counter, device): in-place
# edits through torch (`m.copy_(..)`, `m[0, 0] = ..`, `m.mul_(..)`) bump the version counter and repack the blocks.  Writes
# that bypass the counter -- `m.data.copy_(..)`, a numpy array sharing a CPU tensor's memory -- are invisible to it and would
# render with the packed (stale) matrices: build new tensors for new cameras, or switch the cache off
# (GSR_VIEW_CACHE=0 in the environment, or diff_gaussian_rasterization.set_view_cache(False)): the blocks are then packed
# on every call, as the reference's caller does.  Tensors created under torch.inference_mode() carry no version counter: a
# settings list that contains one is never cached.
import os as _os

_VIEW_BLOCKS = {}          # key -> (view, proj, cam, the source tensors kept alive so that their addresses cannot be reused)
_VIEW_BLOCKS_MAX = 32
_BG_SAME = {}              # (key of a, key of b) -> the two background tensors hold the same three values
_VIEW_CACHE_ON = _os.environ.get("GSR_VIEW_CACHE", "1") != "0"


def set_view_cache(on):
    """Switch the packed-view-block cache of rasterize_views on or off (off: pack the per-view matrices on every call)."""
    global _VIEW_CACHE_ON
    _VIEW_CACHE_ON = bool(on)
    if not on:
        _VIEW_BLOCKS.clear()
        _BG_SAME.clear()


def _tkey(t):
    """Identity of a tensor's current contents as far as torch tracks it, or None when it does not (inference tensors)."""
    try:
        ver = t._version
    except RuntimeError:
        return None
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), ver, t.device.type, t.device.index)


def _same_background(a, b):
    if a is b or (a.data_ptr() == b.data_ptr() and a.device == b.device and a.shape == b.shape and a.stride() == b.stride()):
        return True
    ka, kb = _tkey(a), _tkey(b)
    if not _VIEW_CACHE_ON or ka is None or kb is None:
        return torch.equal(a.detach().cpu(), b.detach().cpu())
    k = ka + kb
    r = _BG_SAME.get(k)
    if r is None:
        if len(_BG_SAME) >= 256:
            _BG_SAME.clear()
        r = (torch.equal(a.detach().cpu(), b.detach().cpu()), a, b)     # one host comparison per pair of tensors, ever
        _BG_SAME[k] = r
    return r[0]


def _pack_views(settings_list, device):
    view = torch.stack([s.viewmatrix.reshape(4, 4).to(device) for s in settings_list], 0).contiguous()
    proj = torch.stack([s.projmatrix.reshape(4, 4).to(device) for s in settings_list], 0).contiguous()
    cam = torch.stack([s.campos.reshape(3).to(device) for s in settings_list], 0).contiguous()
    return view, proj, cam


def _check_views_agree(settings_list):
    s0 = settings_list[0]
    for s in settings_list[1:]:
        if (s.image_height, s.image_width, s.tanfovx, s.tanfovy, s.scale_modifier, s.sh_degree, s.prefiltered) != (
                s0.image_height, s0.image_width, s0.tanfovx, s0.tanfovy, s0.scale_modifier, s0.sh_degree, s0.prefiltered) or \
                not _same_background(s.bg, s0.bg):
            raise Exception("rasterize_views: the views of a batch must share image size, tan(fov), background, scale "
                            "modifier, SH degree and the prefiltered flag")


def _stack_views(settings_list, device):
    _check_views_agree(settings_list)
    _C._require_hip(device)
    keys = [_tkey(t) for s in settings_list for t in (s.viewmatrix, s.projmatrix, s.campos)]
    if not _VIEW_CACHE_ON or any(k is None for k in keys):
        return _pack_views(settings_list, device)
    key = (device.type, device.index) + tuple(keys)
    hit = _VIEW_BLOCKS.get(key)
    cur = torch.cuda.current_stream(device)
    if hit is None:
        view, proj, cam = _pack_views(settings_list, device)
        # other host threads may pick the blocks up on other streams: they wait (on the device) for this event, nobody waits
        # on the host
        ev = torch.cuda.Event()
        ev.record(cur)
        if len(_VIEW_BLOCKS) >= _VIEW_BLOCKS_MAX:
            _VIEW_BLOCKS.pop(next(iter(_VIEW_BLOCKS)))
        hit = (view, proj, cam, [(s.viewmatrix, s.projmatrix, s.campos) for s in settings_list], ev, cur.cuda_stream)
        _VIEW_BLOCKS[key] = hit
    elif hit[5] != cur.cuda_stream:
        cur.wait_event(hit[4])
    return hit[0], hit[1], hit[2]


def _forward_args(settings_list, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, view, proj, cam):
    """the 19 positional arguments of _native.rasterize_gaussians_batch for the views of settings_list"""
    rs = settings_list[0]
    return (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, view, proj,
            rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh, rs.sh_degree, cam, rs.prefiltered,
            any(s.debug for s in settings_list))


def _arena_args(rs, saved, *middle):
    """The leading arguments of the native calls that run on the arenas of a view-batch forward, from the thirteen tensors every such
    forward saves (the order of _RasterizeGaussiansViews.forward's save_for_backward): through geomBuffer, with `middle` where the
    backwards take dL/d image and the followers (backward_cameras, backward_view_stats, contrib_stats) the image's height and width."""
    colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, _binning, _img, view, proj, cam = saved[:13]
    return (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, view, proj, rs.tanfovx,
            rs.tanfovy) + middle + (sh, rs.sh_degree, cam, geomBuffer)


class _RasterizeGaussiansViews(torch.autograd.Function):
    """The view batch: forward and colour backward of every view-batch Function but the channels one, which saves more and calls
    other entries.  cameras: (view, proj, cam) blocks that take the place of the settings' own matrix fields (not part of apply's
    arguments: _RasterizeGaussiansViewsCameras hands them over)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings_list, cameras=None):
        view, proj, cam = cameras if cameras is not None else _stack_views(settings_list, means3D.device)
        counts, color, radii, geomBuffer, binningBuffer, imgBuffer = _C.rasterize_gaussians_batch(
            *_forward_args(settings_list, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, view, proj, cam),
            need_backward=any(ctx.needs_input_grad))
        ctx.raster_settings = settings_list[0]
        ctx.num_rendered = counts
        ctx.opacity_shape = tuple(opacities.shape)
        ctx.det_pairs = _C.last_list_pairs(len(counts)) if means3D.shape[0] != 0 and _C.deterministic_active() else None
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
                              imgBuffer, view, proj, cam)
        ctx.mark_non_differentiable(radii)
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _):
        rs, saved = ctx.raster_settings, ctx.saved_tensors
        colors_precomp, _m, scales, rotations, cov3Ds_precomp, _r, sh, _g, binningBuffer, imgBuffer = saved[:10]
        grads = _C.rasterize_gaussians_backward_batch(*_arena_args(rs, saved, grad_out_color), binningBuffer, imgBuffer, rs.debug,
                                                      deterministic=_C.deterministic_active(), pairs=ctx.det_pairs)
        return _input_grads(grads, ctx, sh, colors_precomp, scales, rotations, cov3Ds_precomp, None)


def rasterize_views(means3D, means2D, opacities, settings_list, shs=None, colors_precomp=None, scales=None, rotations=None,
                    cov3D_precomp=None):
    """GaussianRasterizer.forward for a LIST of GaussianRasterizationSettings (views of one cloud) in one call.
    Returns (colors [V,3,H,W], radii [V,P]); gradients of the shared inputs are the sums over the views."""
    if len(settings_list) == 0:
        raise Exception("rasterize_views: empty settings list")
    _check_sources(shs, colors_precomp, scales, rotations, cov3D_precomp)
    shs, colors_precomp, scales, rotations, cov3D_precomp = _absent_as_empty(shs, colors_precomp, scales, rotations, cov3D_precomp)
    return _RasterizeGaussiansViews.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                          list(settings_list))


class DensityStats:
    """The running accumulators of adaptive density control (split / clone / prune) for a cloud of P Gaussians, fed by
    rasterize_views_stats: per Gaussian, over every view of every backward since the last reset(),
        grad_norm_sum  float32 [P]  sum of the norms of the screen-space gradient dL/dmean2D of each view (pixel units)
        visible_views  int32   [P]  views in which the Gaussian was visible (radius > 0)
        max_radius     int32   [P]  its largest screen radius
    keep_view_grads: each backward also leaves its per-view gradients in `view_grads`, a dict of mean2D [V,P,2], color [V,P,3] and
    opacity [V,P] (None until such a backward has run; replaced, not accumulated, by the next one)."""

    def __init__(self, P, device, keep_view_grads=False):
        self.P, self.device, self.keep_view_grads = int(P), torch.device(device), bool(keep_view_grads)
        self.grad_norm_sum = torch.zeros((self.P,), dtype=torch.float32, device=self.device)
        self.visible_views = torch.zeros((self.P,), dtype=torch.int32, device=self.device)
        self.max_radius = torch.zeros((self.P,), dtype=torch.int32, device=self.device)
        self.view_grads = None

    def reset(self):
        """Zero the three accumulators in place and drop the per-view gradients (after a densification step)."""
        self.grad_norm_sum.zero_()
        self.visible_views.zero_()
        self.max_radius.zero_()
        self.view_grads = None

    def mean_grad(self):
        """grad_norm_sum / max(visible_views, 1): the average screen-space gradient norm per view that saw the Gaussian."""
        return self.grad_norm_sum / self.visible_views.clamp(min=1).to(torch.float32)


class _RasterizeGaussiansViewsStats(torch.autograd.Function):
    """_RasterizeGaussiansViews whose backward also feeds a DensityStats: the same native calls, so images, radii and gradients are
    those of rasterize_views bit for bit, and one more call after the colour backward (C ABI gsr_backward_view_stats)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings_list, stats):
        ctx.stats = stats
        return _RasterizeGaussiansViews.forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                                cov3Ds_precomp, settings_list)

    @staticmethod
    def backward(ctx, grad_out_color, _):
        grads = _RasterizeGaussiansViews.backward(ctx, grad_out_color, _)
        rs, st = ctx.raster_settings, ctx.stats
        # the gradient records of the backward above are still in the arenas: one pass over them per Gaussian
        g = _C.backward_view_stats(*_arena_args(rs, ctx.saved_tensors, rs.image_height, rs.image_width), rs.debug, accumulate=True,
                                   grad_norm_sum=st.grad_norm_sum, visible_views=st.visible_views, max_radius=st.max_radius,
                                   view_grads=st.keep_view_grads)
        if st.keep_view_grads:
            st.view_grads = dict(mean2D=g[0], color=g[1], opacity=g[2])
        return grads + (None,)


def rasterize_views_stats(means3D, means2D, opacities, settings_list, stats, shs=None, colors_precomp=None, scales=None,
                          rotations=None, cov3D_precomp=None):
    """rasterize_views for a training loop with adaptive density control: the same (colors [V,3,H,W], radii [V,P]) and the same
    gradients, bit for bit, and every backward adds its views to `stats` (a DensityStats for this cloud): the sum over the views of
    the NORM of each view's dL/dmean2D -- which the summed means2D.grad cannot give: gradients from opposite views cancel in it --,
    the visibility count and the largest radius; with stats.keep_view_grads also the per-view dL/dmean2D, dL/dcolor, dL/dopacity.
    Without an input that needs a gradient no backward runs and `stats` stays as it is."""
    if len(settings_list) == 0:
        raise Exception("rasterize_views_stats: empty settings list")
    _check_sources(shs, colors_precomp, scales, rotations, cov3D_precomp)
    if not isinstance(stats, DensityStats):
        raise Exception("rasterize_views_stats: stats must be a DensityStats")
    if stats.P != means3D.shape[0] or stats.grad_norm_sum.device != means3D.device:
        raise Exception("rasterize_views_stats: stats was built for %d Gaussians on %s, the cloud has %d on %s"
                        % (stats.P, stats.grad_norm_sum.device, means3D.shape[0], means3D.device))
    shs, colors_precomp, scales, rotations, cov3D_precomp = _absent_as_empty(shs, colors_precomp, scales, rotations, cov3D_precomp)
    return _RasterizeGaussiansViewsStats.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                               list(settings_list), stats)


class ContributionStats:
    """The running accumulators of importance-based pruning and compaction for a cloud of P Gaussians, fed by
    rasterize_views_contrib: per Gaussian, over every pixel of every view since the last reset(), with w = alpha T the blend weight
    of the Gaussian at a pixel it contributes to,
        weight_sum      float32 [P]  sum of w (times the pixel's weight, with a weight map)
        weight_max      float32 [P]  largest w (times the pixel's weight)
        pixel_count     int32   [P]  pixels it contributed to
        dominant_count  int32   [P]  pixels at which its w was the largest
    and pixels_seen, a Python int: V * H * W added per call, for normalising."""

    def __init__(self, P, device):
        self.P, self.device = int(P), torch.device(device)
        self.weight_sum = torch.zeros((self.P,), dtype=torch.float32, device=self.device)
        self.weight_max = torch.zeros((self.P,), dtype=torch.float32, device=self.device)
        self.pixel_count = torch.zeros((self.P,), dtype=torch.int32, device=self.device)
        self.dominant_count = torch.zeros((self.P,), dtype=torch.int32, device=self.device)
        self.pixels_seen = 0

    def reset(self):
        """Zero the four accumulators in place and pixels_seen (after a pruning step)."""
        self.weight_sum.zero_()
        self.weight_max.zero_()
        self.pixel_count.zero_()
        self.dominant_count.zero_()
        self.pixels_seen = 0

    def mean_weight(self):
        """weight_sum / max(pixel_count, 1): the average blend weight over the pixels the Gaussian contributed to."""
        return self.weight_sum / self.pixel_count.clamp(min=1).to(torch.float32)


def rasterize_views_contrib(means3D, means2D, opacities, settings_list, stats, pixel_weights=None, shs=None, colors_precomp=None,
                            scales=None, rotations=None, cov3D_precomp=None):
    """rasterize_views for an importance-pruning pass: the same (colors [V,3,H,W], radii [V,P]), bit for bit, under no_grad, and the
    views' blend weights added to `stats` (a ContributionStats for this cloud) by one more native call on the forward's arenas
    (C ABI gsr_contrib_stats).  pixel_weights: float32 [V,H,W] on the cloud's device, the weight of every pixel (a value that is not
    > 0 masks its pixel out), or None for 1 everywhere."""
    if len(settings_list) == 0:
        raise Exception("rasterize_views_contrib: empty settings list")
    _check_sources(shs, colors_precomp, scales, rotations, cov3D_precomp)
    if not isinstance(stats, ContributionStats):
        raise Exception("rasterize_views_contrib: stats must be a ContributionStats")
    if stats.P != means3D.shape[0] or stats.weight_sum.device != means3D.device:
        raise Exception("rasterize_views_contrib: stats was built for %d Gaussians on %s, the cloud has %d on %s"
                        % (stats.P, stats.weight_sum.device, means3D.shape[0], means3D.device))
    rs, V = settings_list[0], len(settings_list)
    if pixel_weights is not None and (not isinstance(pixel_weights, torch.Tensor) or pixel_weights.dtype != torch.float32
                                      or tuple(pixel_weights.shape) != (V, rs.image_height, rs.image_width)
                                      or pixel_weights.device != means3D.device):
        raise Exception("rasterize_views_contrib: pixel_weights must be a float32 tensor of shape [%d, %d, %d] on %s"
                        % (V, rs.image_height, rs.image_width, means3D.device))
    shs, colors_precomp, scales, rotations, cov3D_precomp = _absent_as_empty(shs, colors_precomp, scales, rotations, cov3D_precomp)
    with torch.no_grad():
        view, proj, cam = _stack_views(settings_list, means3D.device)
        fwd = _forward_args(settings_list, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, view, proj, cam)
        _counts, color, radii, geomBuffer, binningBuffer, imgBuffer = _C.rasterize_gaussians_batch(*fwd, need_backward=False)
        # (what a Function would have saved, in its order)
        saved = (colors_precomp, means3D, scales, rotations, cov3D_precomp, radii, shs, geomBuffer, binningBuffer, imgBuffer, view, proj, cam)
        _C.contrib_stats(*_arena_args(rs, saved, rs.image_height, rs.image_width), binningBuffer, imgBuffer, debug=fwd[-1],
                         accumulate=True, pixel_weights=pixel_weights, weight_sum=stats.weight_sum, weight_max=stats.weight_max,
                         pixel_count=stats.pixel_count, dominant_count=stats.dominant_count)
        stats.pixels_seen += V * int(rs.image_height) * int(rs.image_width)
    return color, radii


class _RasterizeGaussiansViewsCameras(torch.autograd.Function):
    """_RasterizeGaussiansViews with the cameras as autograd inputs: view / proj [V,4,4] and cam [V,3] on the device instead of the
    settings' own matrix fields.  The same native calls, so images and cloud gradients are those of rasterize_views bit for bit;
    the camera gradients come from one more call after the colour backward (C ABI gsr_backward_cameras)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, view, proj, cam,
                settings_list):
        _check_views_agree(settings_list)
        device = means3D.device
        _C._require_hip(device)
        ctx.cam_shapes = (tuple(view.shape), tuple(proj.shape), tuple(cam.shape))
        cameras = (_C._f32c(view, device, "viewmatrices"), _C._f32c(proj, device, "projmatrices"), _C._f32c(cam, device, "campos"))
        return _RasterizeGaussiansViews.forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                                cov3Ds_precomp, settings_list, cameras)

    @staticmethod
    def backward(ctx, grad_out_color, _):
        grads = _RasterizeGaussiansViews.backward(ctx, grad_out_color, _)
        g_cam = (None, None, None)
        if any(ctx.needs_input_grad[8:11]):
            rs = ctx.raster_settings
            # the gradient records of the backward above are still in the arenas: one reduction over them per view
            g = _C.backward_cameras(*_arena_args(rs, ctx.saved_tensors, rs.image_height, rs.image_width), rs.debug)
            g_cam = tuple(t.reshape(shape) if need else None
                          for t, shape, need in zip(g, ctx.cam_shapes, ctx.needs_input_grad[8:11]))
        return grads[:-1] + g_cam + (None,)   # (the cameras' gradients go between the cloud's and the settings' None)


def rasterize_views_cameras(means3D, means2D, opacities, settings_list, viewmatrices, projmatrices, campos, shs=None,
                            colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
    """rasterize_views with differentiable cameras (pose refinement): viewmatrices / projmatrices [V,4,4] (transposed like the
    settings' fields) and campos [V,3], on the device, are autograd inputs and take the place of the settings' own matrix fields,
    which are ignored; settings_list supplies V and the fields the views share.  Returns (colors [V,3,H,W], radii [V,P]): the images
    and the cloud's gradients of rasterize_views with the same matrices, bit for bit.  The camera gradients follow the conventions of
    include/gsr.h gsr_backward_cameras: depth order, culling and tile lists are not differentiated, projmatrix rows the rasterizer
    never reads get zeros, campos gets a gradient through the SH view direction only."""
    if len(settings_list) == 0:
        raise Exception("rasterize_views_cameras: empty settings list")
    _check_sources(shs, colors_precomp, scales, rotations, cov3D_precomp)
    V = len(settings_list)
    if viewmatrices.numel() != 16 * V or projmatrices.numel() != 16 * V or campos.numel() != 3 * V:
        raise Exception("rasterize_views_cameras: viewmatrices and projmatrices must be [V,4,4] and campos [V,3] for the V views of "
                        "settings_list")
    shs, colors_precomp, scales, rotations, cov3D_precomp = _absent_as_empty(shs, colors_precomp, scales, rotations, cov3D_precomp)
    return _RasterizeGaussiansViewsCameras.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                                 viewmatrices, projmatrices, campos, list(settings_list))


class _RasterizeGaussiansViewsChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, extra, extra_hi, bg_extra,
                extra_view_scale, settings_list, nx_user):
        rs = settings_list[0]
        view, proj, cam = _stack_views(settings_list, means3D.device)
        need_backward = any(ctx.needs_input_grad)
        values = (extra, extra_hi) if extra_hi.numel() != 0 else extra
        xs = None if extra_view_scale.numel() == 0 else extra_view_scale
        counts, color, radii, geomBuffer, binningBuffer, imgBuffer, out_extra = _C.rasterize_gaussians_batch(
            *_forward_args(settings_list, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, view, proj, cam),
            need_backward=need_backward, extra=(values, xs, bg_extra))
        ctx.raster_settings = rs
        ctx.opacity_shape = tuple(opacities.shape)
        ctx.nx_user = nx_user
        ctx.xstate = _C.extra_state(geomBuffer)
        # the deterministic channels backward sizes its scratch block by the lists' extent (same host thread as the forward call)
        ctx.det_channels = get_deterministic_channels()
        ctx.det_pairs = _C.last_list_pairs(len(settings_list)) if ctx.det_channels and need_backward and means3D.shape[0] != 0 else None
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
                              imgBuffer, view, proj, cam, extra, extra_hi, bg_extra, extra_view_scale)
        ctx.mark_non_differentiable(radii)
        return color, radii, out_extra[:, :nx_user]

    @staticmethod
    def backward(ctx, grad_out_color, _, grad_out_extra):
        rs, saved = ctx.raster_settings, ctx.saved_tensors
        colors_precomp, _m, scales, rotations, cov3Ds_precomp, _r, sh, _g, binningBuffer, imgBuffer = saved[:10]
        extra, extra_hi, bg_extra, extra_view_scale = saved[13:]
        split = extra_hi.numel() != 0
        nx = 8 if split else extra.shape[-1]
        V = grad_out_color.shape[0]
        if grad_out_extra.shape[1] != nx:   # (channels padded by rasterize_views_channels get no gradient to pass on)
            grad_out_extra = torch.cat([grad_out_extra, grad_out_extra.new_zeros((V, nx - grad_out_extra.shape[1]) +
                                                                                 tuple(grad_out_extra.shape[2:]))], 1)
        values = (extra, extra_hi) if split else extra
        xs = None if extra_view_scale.numel() == 0 else extra_view_scale
        g = _C.rasterize_gaussians_backward_channels_batch(
            *_arena_args(rs, saved, grad_out_color), binningBuffer, imgBuffer, rs.debug, (values, xs, bg_extra), grad_out_extra,
            state=ctx.xstate, deterministic=ctx.det_channels, pairs=ctx.det_pairs)
        g_lo, g_hi = g[8] if split else (g[8], None)
        return _input_grads(g[:8], ctx, sh, colors_precomp, scales, rotations, cov3Ds_precomp, g_lo, g_hi, None, None, None, None)


def rasterize_views_channels(means3D, means2D, opacities, settings_list, extra, bg_extra, extra_view_scale=None, shs=None,
                             colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
    """rasterize_views that also composites extra per-Gaussian channels with the colour's alphas, differentiably (C ABI
    gsr_forward_batch_channels_train / gsr_backward_batch_channels).  Returns (colors [V,3,H,W], radii [V,P],
    extra_images [V,nx,H,W]): extra_images[v][k] = sum_i extra[i][k] * extra_view_scale[v][k] * alpha_i T_i + T_final bg_extra[k],
    what a rasterize_views call with those values as colors_precomp and bg_extra as background renders.
    extra: [P,nx] shared by the views, [V,P,nx] one array per view, or the pair ([P,4], [V,P,4]) (channels 0..3 shared, 4..7 per
    view); nx = 1..8 (padded to 4 / 8 with zero channels).  bg_extra [nx]; extra_view_scale [V,nx] or None.  Gradients flow to
    `extra` as to every input rasterize_views differentiates; bg_extra and extra_view_scale get none (like the background)."""
    if len(settings_list) == 0:
        raise Exception("rasterize_views_channels: empty settings list")
    # the atomic channels backward adds dL/d extra with float atomics of its own; the deterministic one (include/gsr.h
    # gsr_backward_batch_channels_det) is behind a switch of its own, set_deterministic_channels: while that is off, the colour
    # backward's switches refuse this call as they always did
    _why = ("rasterize_views_channels has no deterministic backward (the extra channels' gradients are accumulated with float "
            "atomics) unless diff_gaussian_rasterization.set_deterministic_channels(True) selects the deterministic channels "
            "backward; or render the channels as colours through rasterize_views, or switch the deterministic path off")
    if get_deterministic_channels():
        pass
    elif get_deterministic() is True:
        raise RuntimeError(_why + ": diff_gaussian_rasterization.set_deterministic(False / None)")
    elif get_deterministic() is None and torch.are_deterministic_algorithms_enabled():
        if torch.is_deterministic_algorithms_warn_only_enabled():
            import warnings
            warnings.warn(_why, UserWarning)
        else:
            raise RuntimeError(_why + ": torch.use_deterministic_algorithms(True, warn_only=True) or set_deterministic(False)")
    _check_sources(shs, colors_precomp, scales, rotations, cov3D_precomp)
    shs, colors_precomp, scales, rotations, cov3D_precomp = _absent_as_empty(shs, colors_precomp, scales, rotations, cov3D_precomp)
    V, P = len(settings_list), means3D.shape[0]
    e = _ABSENT
    dev = means3D.device
    if isinstance(extra, (tuple, list)):
        lo, hi = extra
        if tuple(lo.shape) != (P, 4) or tuple(hi.shape) != (V, P, 4):
            raise Exception("rasterize_views_channels: split extra channels must have shapes (P, 4) and (V, P, 4)")
        nx_user, nx = 8, 8
    else:
        lo, hi = extra, e
        if lo.dim() not in (2, 3) or lo.shape[-2] != P or (lo.dim() == 3 and lo.shape[0] != V) or not 1 <= lo.shape[-1] <= 8:
            raise Exception("rasterize_views_channels: extra must have shape (P, nx) or (V, P, nx) with nx in 1..8")
        nx_user = int(lo.shape[-1])
        nx = 4 if nx_user <= 4 else 8
        if nx != nx_user:   # zero channels up to a quad (torch ops: the gradient is sliced back by autograd)
            lo = torch.cat([lo, lo.new_zeros(tuple(lo.shape[:-1]) + (nx - nx_user,))], -1)
    bg_extra = bg_extra.detach().reshape(-1).to(device=dev, dtype=torch.float32)
    if bg_extra.numel() != nx_user:
        raise Exception("rasterize_views_channels: bg_extra must have one value per extra channel")
    if nx != nx_user:
        bg_extra = torch.cat([bg_extra, bg_extra.new_zeros(nx - nx_user)])
    if extra_view_scale is None:
        xs = e
    else:
        xs = extra_view_scale.detach().to(device=dev, dtype=torch.float32).reshape(V, nx_user)
        if nx != nx_user:
            xs = torch.cat([xs, xs.new_ones((V, nx - nx_user))], 1)
        xs = xs.contiguous()
    return _RasterizeGaussiansViewsChannels.apply(
        means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, lo.contiguous(),
        hi if hi is e else hi.contiguous(), bg_extra.contiguous(), xs, list(settings_list), nx_user)
