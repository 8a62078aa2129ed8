"""Everything between a test and diff_gaussian_rasterization._native: how the 19 forward arguments are built, how the calls that
follow a forward take them, and the library's switches.  Importable without torch, the built library or a device (torch and _native
are imported inside the functions).

  to_device                                  numpy -> device tensor
  BG .. DEBUG                                names of the 19 positions of rasterize_gaussians(_batch)'s argument list
  scene_args                                 the argument list for views of one cloud given as oracle Scenes
  cloud_views / circle_scene                 the synthetic cloud and circle cameras (circle_scene: all twelve cameras at n_views = 12)
  cloud_args / batch_args                    their argument list (a list, bg required / a tuple, white background)
  one_view                                   a batch's argument list with view v's camera alone
  scene_settings / unit_settings             GaussianRasterizationSettings of oracle Scenes; of an 8 x 8 identity view on the host
  colour_backward_args / channels_backward_args / follower_args / contrib_stats_args / recolor_args
                                             a forward's arguments and run tuple, permuted for the call that follows it
  colour_backward / channels_backward        forward + backward, numpy gradient dicts
  longest_list                               the longest tile list of a batch
  alloc_arenas / forward_on / stage_pair_on / colour_det_backward_on / ckpt_region
                                             the raw calls on caller-given arenas: a zero-filled set, a (channels-train, resumed)
                                             forward, the stage pair, the deterministic colour backward with a given scratch block,
                                             and the bytes of a view's slice-boundary states inside the binning arena
  render_math / half_views / train_math / moments / reference_lists
                                             a switch set for a block and restored whatever happens inside
  RGB_TOL / RENDER_SCENES / renders          the inference renders of the test scenes in both arithmetic modes, rendered once"""
import contextlib
import functools

import numpy as np

import util

BG, MEANS3D, COLORS, OPACITIES, SCALES, ROTATIONS, SCALE_MODIFIER, COV3D, VIEWMATRIX, PROJMATRIX, TANFOVX, TANFOVY, HEIGHT, WIDTH, \
    SHS, SH_DEGREE, CAMPOS, PREFILTERED, DEBUG = range(19)


def to_device(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- the forward's arguments ------------------------------------------------------------------------------------------------------
def scene_args(scenes, dev):
    """rasterize_gaussians_batch arguments for views of one cloud, given as oracle Scenes"""
    import torch
    s = scenes[0]
    e = torch.empty(0)
    a = lambda x: e if x is None else to_device(x, dev)  # noqa: E731
    vm = to_device(np.stack([x.viewmatrix.reshape(4, 4) for x in scenes]), dev)
    pm = to_device(np.stack([x.projmatrix.reshape(4, 4) for x in scenes]), dev)
    cp = to_device(np.stack([x.campos.reshape(3) for x in scenes]), dev)
    return [a(s.bg), a(s.means3D), a(s.colors_precomp), a(s.opacities.reshape(-1, 1)), a(s.scales), a(s.rotations),
            float(s.scale_modifier), a(s.cov3D_precomp), vm, pm, s.tanfovx, s.tanfovy, s.H, s.W, a(s.shs),
            int(s.sh_degree) if s.shs is not None else 0, cp, False, False]


def cloud_views(n_views=3, P=12000, W=208, H=176, profile="training", twelve=False):
    """One cloud, n_views circle cameras (view 0 is axis aligned: depth ties on the voxelised cloud).  The cameras are 0, 1, 5, 7, 10
    of the circle of twelve, cut to n_views; twelve: all twelve for n_views = 12."""
    from pcrender import camera, synth
    cloud = synth.make_cloud("synth-THuman-256", seed=0, P=P)
    g = synth.make_gaussians(cloud, profile=profile, seed=1)
    views = camera.circle_views(12, fov_deg=45.0, width_px=W, height_px=H)
    pick = list(range(12)) if twelve and n_views == 12 else [0, 1, 5, 7, 10][:n_views]
    return g, [views[i] for i in pick], W, H


def circle_scene(n_views, P=12000, W=208, H=176, bg=(0.0, 0.0, 0.0)):
    return cloud_views(n_views, P=P, W=W, H=H, twelve=True)


def cloud_args(g, views, W, H, dev, bg):
    import torch
    e = torch.empty(0)
    vm = torch.stack([v["viewmatrix"] for v in views]).to(dev)
    pm = torch.stack([v["projmatrix"] for v in views]).to(dev)
    cp = torch.stack([v["campos"] for v in views]).to(dev)
    return [to_device(np.asarray(bg, np.float32), dev), to_device(g["means3D"], dev), e, to_device(g["opacities"], dev),
            to_device(g["scales"], dev), to_device(g["rotations"], dev), 1.0, e, vm, pm, views[0]["tanfovx"], views[0]["tanfovy"], H, W,
            to_device(g["shs"], dev), g["sh_degree"], cp, False, False]


def batch_args(g, views, W, H, dev, bg=(1, 1, 1)):
    return tuple(cloud_args(g, views, W, H, dev, bg))


def scene_settings(scenes, dev):
    """one GaussianRasterizationSettings per oracle Scene"""
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return [GaussianRasterizationSettings(
        image_height=s.H, image_width=s.W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=to_device(s.bg, dev), scale_modifier=1.0,
        viewmatrix=to_device(s.viewmatrix.reshape(4, 4), dev), projmatrix=to_device(s.projmatrix.reshape(4, 4), dev),
        sh_degree=s.sh_degree, campos=to_device(s.campos, dev), prefiltered=False, debug=False) for s in scenes]


def unit_settings():
    """settings of an 8 x 8 view with identity matrices, on the host: for calls that are refused before they look at them"""
    import torch
    import diff_gaussian_rasterization as d
    return d.GaussianRasterizationSettings(
        image_height=8, image_width=8, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False,
        debug=False)


def one_view(args, v):
    a = list(args)
    a[VIEWMATRIX], a[PROJMATRIX], a[CAMPOS] = args[VIEWMATRIX][v], args[PROJMATRIX][v], args[CAMPOS][v]
    return a


# ---- the calls that follow a forward: `run` = (counts, color, radii, geom, binning, img, ...) -------------------------------------
def colour_backward_args(args, run, dL, scale_modifier=None):
    """rasterize_gaussians_backward_batch's positional arguments; scale_modifier: a value other than the forward's"""
    radii, geom, binning, img = run[2:6]
    return (args[BG], args[MEANS3D], radii, args[COLORS], args[SCALES], args[ROTATIONS],
            args[SCALE_MODIFIER] if scale_modifier is None else scale_modifier, args[COV3D], args[VIEWMATRIX], args[PROJMATRIX],
            args[TANFOVX], args[TANFOVY], dL, args[SHS], args[SH_DEGREE], args[CAMPOS], geom, binning, img, False)


def channels_backward_args(args, run, dpix, extra, dx, scale_modifier=None):
    """rasterize_gaussians_backward_channels_batch's positional arguments; extra = (values, view scales, bg_extra)"""
    return colour_backward_args(args, run, dpix, scale_modifier) + (extra, dx)


def follower_args(args, radii, geom, V=None):
    """the positional arguments of backward_cameras and backward_view_stats: the first V views of the batch (default: all)"""
    V = args[VIEWMATRIX].shape[0] if V is None else V
    return (args[BG], args[MEANS3D], None if radii is None else radii[:V], args[COLORS], args[SCALES], args[ROTATIONS],
            args[SCALE_MODIFIER], args[COV3D], args[VIEWMATRIX][:V], args[PROJMATRIX][:V], args[TANFOVX], args[TANFOVY], args[HEIGHT],
            args[WIDTH], args[SHS], args[SH_DEGREE], args[CAMPOS][:V], geom)


def contrib_stats_args(args, run, V=None, radii=True):
    """contrib_stats' positional arguments; radii = False: the call without the forward's radii"""
    return follower_args(args, run[2] if radii else None, run[3], V) + (run[4], run[5])


def recolor_args(args, run, colours=None, campos=None):
    """recolor's positional arguments: precomputed colours, or the arguments' SH table evaluated from campos (default: the forward's)"""
    import torch
    e = torch.empty(0)
    colour = (colours, e, 0, args[CAMPOS]) if colours is not None else (e, args[SHS], args[SH_DEGREE], args[CAMPOS] if campos is None else campos)
    return (args[BG], args[MEANS3D]) + colour + (args[HEIGHT], args[WIDTH], run[0], run[3], run[4], run[5])


def colour_backward(N, args, dL, need_grads=True):
    """forward + backward of plain colour calls (scale modifier 1); returns the numpy gradient dict"""
    run = N.rasterize_gaussians_batch(*args, need_backward=True)
    g = N.rasterize_gaussians_backward_batch(*colour_backward_args(args, run, dL, scale_modifier=1.0))
    return {n: x.detach().cpu().numpy().astype(np.float64) for n, x in zip(util.GRAD_NAMES, g)}


def channels_backward(N, args, x, scale, bgx, dpix, dx, capacity=None):
    """channels forward + backward (scale modifier 1): (gradient dict, dL/d values flat, (counts, color, radii, out_x, geom, binning,
    img)), numpy"""
    import torch
    counts, color, radii, geom, binning, img, out_x = N.rasterize_gaussians_batch(*args, need_backward=True, extra=(x, scale, bgx),
                                                                                 capacity=capacity)
    g = N.rasterize_gaussians_backward_channels_batch(*channels_backward_args(args, (counts, color, radii, geom, binning, img), dpix,
                                                                              (x, scale, bgx), dx, scale_modifier=1.0))
    gp = {n: t.detach().cpu().numpy() for n, t in zip(util.GRAD_NAMES, g[:8])}
    gx = g[8]
    gx = torch.cat([gx[0].reshape(-1), gx[1].reshape(-1)]) if isinstance(gx, tuple) else gx
    return gp, gx.cpu().numpy(), (counts, color, radii, out_x, geom, binning, img)


def longest_list(N, geom, binning, img, counts, P, W, H, V):
    """the longest tile list of the batch (entries): > 1024 means the slices start at recorded chunk boundaries"""
    best = 0
    for v in range(V):
        r = N.query("RANGES", P, W, H, counts[v], geom, binning, img, view=v, n_views=V).reshape(-1, 2).long()
        best = max(best, int((r[:, 1] - r[:, 0]).max()))
    return best


# ---- raw calls on caller-given arenas --------------------------------------------------------------------------------------------
def alloc_arenas(N, P, W, H, V, capacity, dev, nx=0):
    """(geom, binning, img, extra state or None): zero-filled arenas of V views with need_backward, the binning arena for
    `capacity` pairs per view, the extra-state block for nx channels at that capacity"""
    import torch
    z = lambda n: torch.zeros((int(n),), dtype=torch.uint8, device=dev)  # noqa: E731
    return (z(V * N.lib.gsr_geom_bytes(P)), z(V * N.lib.gsr_binning_bytes(int(capacity))), z(V * N.lib.gsr_image_bytes(W, H)),
            z(V * N.lib.gsr_extra_state_bytes(W, H, int(capacity), nx) + 256) if nx else None)


def forward_on(N, args, geom, binning, img, need_backward, resume=0, extra=None, xstate=None, out=None):
    """gsr_forward_batch on the given arenas -- with extra = (values, view scales or None, bg_extra): gsr_forward_batch_channels_train
    into the block xstate (need_backward) or gsr_forward_batch_channels.  Returns (status, run): run = (counts, color, radii, geom,
    binning, img[, out_extra]) like rasterize_gaussians_batch.  out: the output tensors (color, radii, out_extra) of an earlier
    attempt, for a resumed call.  (fp64_pins.raw_forward is the older, narrower form -- colour only, no resume, status asserted,
    counts dropped -- and stays as the tests that import it have it)"""
    import ctypes as C
    import torch
    dev = args[MEANS3D].device
    P, V, H, W = args[MEANS3D].shape[0], args[VIEWMATRIX].numel() // 16, args[HEIGHT], args[WIDTH]
    nx = 0
    if extra is not None:
        nx, layout, xv, xs, xb = N._extra_layout(extra, P, V, dev)
        xv, xs, xb = N._extra_f32(xv, xs, xb, dev)
    if out is None:
        out = (torch.empty((V, 3, H, W), dtype=torch.float32, device=dev), torch.empty((V, P), dtype=torch.int32, device=dev),
               torch.empty((V, nx, H, W), dtype=torch.float32, device=dev) if nx else None)
    color, radii, out_x = out
    p, keep = N._params(*args, need_backward=need_backward)
    counts = (C.c_int64 * V)()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        head = (C.byref(p), V, geom.data_ptr(), geom.numel(), img.data_ptr(), img.numel(), binning.data_ptr(), binning.numel(),
                radii.data_ptr(), color.data_ptr(), counts, int(resume))
        if not nx:
            rc = N.lib.gsr_forward_batch(*head, stream)
        else:
            x = (nx, layout, xv.data_ptr(), None if xs is None else xs.data_ptr(), xb.data_ptr(), out_x.data_ptr())
            if need_backward:
                rc = N.lib.gsr_forward_batch_channels_train(*head, *x, xstate.data_ptr(), xstate.numel(), stream)
            else:
                rc = N.lib.gsr_forward_batch_channels(*head, *x, stream)
    torch.cuda.synchronize()
    del keep
    run = ([int(c) for c in counts], color, radii, geom, binning, img)
    return rc, run + ((out_x,) if nx else ())


def stage_pair_on(N, args, geom, binning, img):
    """gsr_forward_stage1 + gsr_forward_stage2 of ONE view (args with [1,4,4] matrices) on the given arenas; returns the run tuple"""
    import ctypes as C
    import torch
    dev = args[MEANS3D].device
    P, H, W = args[MEANS3D].shape[0], args[HEIGHT], args[WIDTH]
    color = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((1, P), dtype=torch.int32, device=dev)
    p, keep = N._params(*args, need_backward=True)
    n = (C.c_int64 * 1)()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = N.lib.gsr_forward_stage1(C.byref(p), geom.data_ptr(), geom.numel(), img.data_ptr(), img.numel(), radii.data_ptr(), n, stream)
        assert rc == 0, N.lib.gsr_last_error()
        rc = N.lib.gsr_forward_stage2(C.byref(p), geom.data_ptr(), geom.numel(), binning.data_ptr(), binning.numel(), img.data_ptr(),
                                      img.numel(), n[0], color.data_ptr(), stream)
        assert rc == 0, N.lib.gsr_last_error()
    torch.cuda.synchronize()
    del keep
    return ([int(n[0])], color, radii, geom, binning, img)


def colour_det_backward_on(N, args, run, dL, scratch):
    """gsr_backward_batch_det on the arenas of `run` with the caller's scratch block: the numpy gradient dict"""
    import torch
    a = colour_backward_args(args, run, dL)
    dev = args[MEANS3D].device
    with torch.cuda.device(dev):
        p, keep, radii, dpix = N._bwd_inputs(*a[:16], False)
        g = N._grad_tensors(p.P, p.M, dev, args[SCALES].numel() != 0)
        head = N._bwd_head(p, int(dL.shape[0]), radii, N._arena_args(*a[16:19]), dpix, g)
        rc = N.lib.gsr_backward_batch_det(*head, scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, N.lib.gsr_last_error()
    del keep
    return {n: t.cpu().numpy() for n, t in zip(util.GRAD_NAMES, g)}


CKPT_SHIFT = 9            # common.hpp BWD_CHUNK_SHIFT_MIN: the boundary-state area is carved for slices of 512 entries
CKPT_SLOT_BYTES = 4096    # 256 float4 per slot (tests/test_cpu_arena_cases.py holds both to the header)


def ckpt_region(N, binning, V, v):
    """the bytes of view v's slice-boundary states (BinView::ckpt, the last array of a view's binning arena) in a binning arena of
    V views, as a view of the tensor: common.hpp bin_view / bin_capacity_from_bytes restated"""
    per_view = ((binning.numel() - 256) // V) // 256 * 256
    lo, hi = 1, per_view // 16 + 1
    while lo < hi:                              # the largest capacity whose arena fits a view's share
        mid = lo + (hi - lo + 1) // 2
        lo, hi = (mid, hi) if N.lib.gsr_binning_bytes(mid) - 256 <= per_view else (lo, mid - 1)
    end = N.lib.gsr_binning_bytes(lo) - 256
    return binning[v * per_view + end - ((lo >> CKPT_SHIFT) + 2) * CKPT_SLOT_BYTES:v * per_view + end]


# ---- the switches -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _library_switch(setter, value):
    """a gsr_set_* switch of the C ABI (-1 reads it) for the block; the value in force before is restored whatever happens inside.
    value None: the block sets the switch itself"""
    from diff_gaussian_rasterization import _native as N
    was = getattr(N.lib, setter)(-1)
    try:
        assert value is None or getattr(N.lib, setter)(value) == value
        yield
    finally:
        getattr(N.lib, setter)(was)


render_math = functools.partial(_library_switch, "gsr_set_render_math")        # the arithmetic of the inference forwards
train_math = functools.partial(_library_switch, "gsr_set_train_math")          # the arithmetic of the training calls
half_views = functools.partial(_library_switch, "gsr_set_forward_half_views")
moments = functools.partial(_library_switch, "gsr_set_backward_moments")


@contextlib.contextmanager
def reference_lists(on):
    """the reference's full tile lists (True) or the footprint-clipped ones (False) for the block"""
    from diff_gaussian_rasterization import _native as N
    old = N.set_reference_lists(on)
    try:
        yield
    finally:
        N.set_reference_lists(old)


# ---- shared renders ---------------------------------------------------------------------------------------------------------------
RGB_TOL = 1e-4            # the contract's tolerance (north_star)
RENDER_SCENES = ["random_aniso", "sh_deg3", "colors_precomp", "cov3d_precomp", "culled_mix", "all_culled", "voxel_ties",
                 "opaque_early_stop", "capsule_circle", "big_splats", "deep_stack", "one_gaussian"]
_RENDERS = {}


def renders(name, dev):
    """(scene, exact inference forward, fast inference forward) of a test scene: rendered once, shared, never written to"""
    if name not in _RENDERS:
        s = util.build_scene(name)
        with render_math(0):
            exact, _ = util.run_product(s, dev, need_backward=False)
        with render_math(1):
            fast, _ = util.run_product(s, dev, need_backward=False)
        _RENDERS[name] = (s, exact, fast)
    return _RENDERS[name]
