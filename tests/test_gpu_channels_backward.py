"""The channels backward (gsr_forward_batch_channels_train + gsr_backward_batch_channels, diff_gaussian_rasterization.
rasterize_views_channels, pcrender.raster_passes.train_passes).

The extra channels are linear in their values and share the colour's alphas, so one channels forward + backward equals the sum of
plain colour backwards on the same cloud and cameras: one with the real colours and dL_dpix, and one per group of three extra
channels with colors_precomp = those values x view scale, bg = those bg_extra and dL = those dL_dextra planes (per view: V = 1 calls,
since the view scales differ per view).  dL/d extra equals those runs' dL_dcolor (x view scale), summed over the views where the
layout shares the values."""
import numpy as np
import pytest
import torch

import util
from fp64_pins import CHECKED, check_channels_grads as _check
from native_calls import (channels_backward as _channels_bwd, channels_backward_args, circle_scene as _scene, cloud_args as _args,
                          colour_backward as _colour_bwd, longest_list as _long_lists, recolor_args, to_device as _t)

pytestmark = pytest.mark.gpu

NAMES = util.GRAD_NAMES


def _extra_inputs(P, V, nx, layout, dev, seed):
    """values as the forward takes them, and the dense [V][P][nx] values they stand for"""
    rng = np.random.default_rng(seed)
    scale = _t(rng.choice([-1.0, 1.0], (V, nx)).astype(np.float32), dev)
    bgx = _t(rng.uniform(0, 1, nx).astype(np.float32), dev)
    if layout == 0:
        x = _t(rng.normal(0, 1, (P, nx)).astype(np.float32), dev)
        dense = x.unsqueeze(0).expand(V, P, nx)
    elif layout == 1:
        x = _t(rng.normal(0, 1, (V, P, nx)).astype(np.float32), dev)
        dense = x
    else:
        lo = _t(rng.normal(0, 1, (P, 4)).astype(np.float32), dev)
        hi = _t(rng.normal(0, 1, (V, P, 4)).astype(np.float32), dev)
        x = (lo, hi)
        dense = torch.cat([lo.unsqueeze(0).expand(V, P, 4), hi], 2)
    return x, scale, bgx, dense


def _decomposition(N, args, V, P, nx, dense, scale, bgx, dpix, dx):
    """sum of the plain colour backwards that the channels backward must equal; returns (grads, dL/d dense values [V][P][nx])"""
    e = torch.empty(0)
    tot = _colour_bwd(N, args, dpix)
    gx = np.zeros((V, P, nx))
    for k0 in range(0, nx, 3):
        ks = list(range(k0, min(k0 + 3, nx)))
        for v in range(V):
            cols = torch.zeros((P, 3), device=dpix.device)
            cols[:, :len(ks)] = dense[v][:, ks] * scale[v, ks]
            bg = torch.zeros(3, device=dpix.device)
            bg[:len(ks)] = bgx[ks]
            dl = torch.zeros((1, 3) + tuple(dpix.shape[2:]), device=dpix.device)
            dl[0, :len(ks)] = dx[v, ks]
            a = list(args)
            a[0], a[2], a[14] = bg, cols.contiguous(), e
            a[8], a[9], a[16] = args[8][v:v + 1], args[9][v:v + 1], args[16][v:v + 1]
            g = _colour_bwd(N, a, dl.contiguous())
            for n in NAMES:
                if n in ("dL_dcolor", "dL_dsh"):
                    continue
                tot[n] = tot[n] + g[n]
            gx[v][:, ks] = g["dL_dcolor"][:, :len(ks)] * scale[v, ks].cpu().numpy()
    return tot, gx


def _fold(gx, layout, V, P):
    if layout == 0:
        return gx.sum(0)
    if layout == 1:
        return gx
    return np.concatenate([gx[:, :, :4].sum(0).reshape(-1), gx[:, :, 4:].reshape(-1)])



@pytest.mark.parametrize("nx,layout,V", [(4, 0, 1), (4, 1, 2), (8, 0, 2), (8, 1, 1), (8, 2, 2), (8, 2, 12), (4, 0, 12)])
def test_channels_backward_is_the_sum_of_colour_backwards(gpu_device, nx, layout, V):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    # a dense cloud on a small image: tile lists of several thousand entries, so backward slices start at saved boundaries
    g, views, W, H = _scene(V, P=40000, W=128, H=112)
    args = _args(g, views, W, H, dev, bg=(0.3, 0.3, 0.3))
    P = g["means3D"].shape[0]
    x, scale, bgx, dense = _extra_inputs(P, V, nx, layout, dev, seed=nx * 10 + layout + V)
    rng = np.random.default_rng(5)
    dpix = _t(rng.uniform(-1, 1, (V, 3, H, W)).astype(np.float32), dev)
    dx = _t(rng.uniform(-1, 1, (V, nx, H, W)).astype(np.float32), dev)
    gp, gx, (counts, _, _, _, geom, binning, img) = _channels_bwd(N, args, x, scale, bgx, dpix, dx)
    assert _long_lists(N, geom, binning, img, counts, P, W, H, V) > 2048
    go, gxo = _decomposition(N, args, V, P, nx, dense, scale, bgx, dpix, dx)
    _check(gp, go, gx, _fold(gxo, layout, V, P), "nx=%d layout=%d V=%d" % (nx, layout, V))


@pytest.mark.parametrize("name", ["random_aniso", "culled_mix", "colors_precomp"])
def test_channels_backward_on_test_scenes(gpu_device, name):
    """tests/util.build_scene scenes (single view, their own backgrounds), nx = 8 per-view values"""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    s = util.build_scene(name)
    e = torch.empty(0)
    a = lambda x: _t(x, dev)  # noqa: E731
    col = a(s.colors_precomp) if s.colors_precomp is not None else e
    shs = a(s.shs) if s.shs is not None else e
    args = [a(s.bg), a(s.means3D), col, a(s.opacities.reshape(-1, 1)), a(s.scales), a(s.rotations), float(s.scale_modifier), e,
            a(s.viewmatrix.reshape(1, 4, 4)), a(s.projmatrix.reshape(1, 4, 4)), s.tanfovx, s.tanfovy, s.H, s.W, shs,
            int(s.sh_degree) if s.shs is not None else 0, a(s.campos.reshape(1, 3)), False, False]
    P, V, nx = s.means3D.shape[0], 1, 8
    x, scale, bgx, dense = _extra_inputs(P, V, nx, 1, dev, seed=3)
    rng = np.random.default_rng(7)
    dpix = a(rng.uniform(-1, 1, (V, 3, s.H, s.W)).astype(np.float32))
    dx = a(rng.uniform(-1, 1, (V, nx, s.H, s.W)).astype(np.float32))
    gp, gx, _ = _channels_bwd(N, args, x, scale, bgx, dpix, dx)
    go, gxo = _decomposition(N, args, V, P, nx, dense, scale, bgx, dpix, dx)
    _check(gp, go, gx, _fold(gxo, 1, V, P), name)


def test_channels_backward_against_the_reference_build(gpu_device):
    """the same decomposition with the reference's own colour backward as the arbiter (one view per call)"""
    from diff_gaussian_rasterization import _native as N
    ref = util.reference_build()
    dev = gpu_device
    V, nx = 2, 4
    g, views, W, H = _scene(V, P=8000, W=96, H=80)
    bg = (0.0, 0.0, 0.0)
    args = _args(g, views, W, H, dev, bg)
    P = g["means3D"].shape[0]
    x, scale, bgx, dense = _extra_inputs(P, V, nx, 1, dev, seed=11)
    rng = np.random.default_rng(8)
    dpix = _t(rng.uniform(-1, 1, (V, 3, H, W)).astype(np.float32), dev)
    dx = _t(rng.uniform(-1, 1, (V, nx, H, W)).astype(np.float32), dev)
    gp, gx, _ = _channels_bwd(N, args, x, scale, bgx, dpix, dx)
    tot = {n: 0.0 for n in CHECKED}
    gxo = np.zeros((V, P, nx))
    for v in range(V):
        s = util.scene_from(g, views[v], W, H, bg=bg)
        _, gr = ref.forward_backward(s, dpix[v].cpu().numpy())
        for n in CHECKED:
            tot[n] = tot[n] + np.asarray(gr[n], np.float64).reshape(gp[n].shape)
        for k0 in range(0, nx, 3):
            ks = list(range(k0, min(k0 + 3, nx)))
            gg = dict(g)
            cols = np.zeros((P, 3), np.float32)
            cols[:, :len(ks)] = (dense[v][:, ks] * scale[v, ks]).cpu().numpy()
            gg["colors_precomp"] = cols
            b3 = np.zeros(3, np.float32)
            b3[:len(ks)] = bgx[ks].cpu().numpy()
            s = util.scene_from(gg, views[v], W, H, bg=b3, mode="colors")
            dl = np.zeros((3, H, W), np.float32)
            dl[:len(ks)] = dx[v, ks].cpu().numpy()
            _, gr = ref.forward_backward(s, dl)
            for n in CHECKED:
                if n in ("dL_dcolor", "dL_dsh"):
                    continue
                tot[n] = tot[n] + np.asarray(gr[n], np.float64).reshape(gp[n].shape)
            gxo[v][:, ks] = np.asarray(gr["dL_dcolor"], np.float64).reshape(P, 3)[:, :len(ks)] * scale[v, ks].cpu().numpy()
    _check(gp, tot, gx, gxo, "vs reference build")


@pytest.mark.parametrize("nx,layout", [(4, 0), (8, 2)])
def test_forward_outputs_unchanged_and_retry_gives_the_same_gradients(gpu_device, nx, layout):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    V = 3
    g, views, W, H = _scene(V)
    args = _args(g, views, W, H, dev, bg=(0.5, 0.5, 0.5))
    P = g["means3D"].shape[0]
    x, scale, bgx, _ = _extra_inputs(P, V, nx, layout, dev, seed=2)
    a = N.rasterize_gaussians_batch(*args, need_backward=False, extra=(x, scale, bgx))
    b = N.rasterize_gaussians_batch(*args, need_backward=True, extra=(x, scale, bgx))
    assert N.extra_state(b[3]) is not None and N.extra_state(a[3]) is None
    assert a[0] == b[0]
    for i in (1, 2, 6):
        assert torch.equal(a[i], b[i]), i
    rng = np.random.default_rng(4)
    dpix = _t(rng.uniform(-1, 1, (V, 3, H, W)).astype(np.float32), dev)
    dx = _t(rng.uniform(-1, 1, (V, nx, H, W)).astype(np.float32), dev)
    g1, gx1, r1 = _channels_bwd(N, args, x, scale, bgx, dpix, dx)
    # a capacity far too small: GSR_RETRY, a larger arena and extra-state block, resume = 1
    g2, gx2, r2 = _channels_bwd(N, args, x, scale, bgx, dpix, dx, capacity=1000)
    assert r2[5].numel() > 0 and torch.equal(r1[1], r2[1]) and torch.equal(r1[3], r2[3])
    _check(g2, {n: g1[n].astype(np.float64) for n in NAMES}, gx2, gx1.astype(np.float64), "retry")


def test_misuse_is_refused_with_a_message(gpu_device):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    V, nx = 2, 8
    g, views, W, H = _scene(V, P=3000, W=64, H=48)
    args = _args(g, views, W, H, dev, bg=(0.0, 0.0, 0.0))
    P = g["means3D"].shape[0]
    x, scale, bgx, _ = _extra_inputs(P, V, nx, 1, dev, seed=1)
    dpix = torch.zeros((V, 3, H, W), device=dev)
    dx = torch.zeros((V, nx, H, W), device=dev)

    def bwd(r, extra, state=None):
        dxe = dx[:, :extra[0].shape[-1]] if not isinstance(extra[0], tuple) else dx
        return N.rasterize_gaussians_backward_channels_batch(*channels_backward_args(args, r, dpix, extra, dxe, 1.0), state=state)

    r = N.rasterize_gaussians_batch(*args, need_backward=True, extra=(x, scale, bgx))
    st = N.extra_state(r[3])
    bwd(r, (x, scale, bgx))                                       # the matching call works
    with pytest.raises(RuntimeError, match="nx = 4"):              # other channel count
        bwd(r, (x[..., :4].contiguous(), scale[:, :4].contiguous(), bgx[:4].contiguous()))
    with pytest.raises(RuntimeError, match="extra_per_view = 0"):  # other layout
        bwd(r, (x[0].contiguous(), scale, bgx))
    # a forward without channels on the same arena
    plain = N.rasterize_gaussians_batch(*args, need_backward=True)
    with pytest.raises(RuntimeError, match="saved no extra channels"):
        bwd(plain, (x, scale, bgx), state=st)
    # a channels forward with need_backward = 0: nothing saved
    r0 = N.rasterize_gaussians_batch(*args, need_backward=False, extra=(x, scale, bgx))
    with pytest.raises(RuntimeError, match="no extra-channel state|saved no extra channels"):
        bwd(r0, (x, scale, bgx))
    with pytest.raises(RuntimeError, match="saved no extra channels"):
        bwd(r0, (x, scale, bgx), state=st)
    # after a recolor
    r = N.rasterize_gaussians_batch(*args, need_backward=True, extra=(x, scale, bgx))
    N.recolor(*recolor_args(args, r, torch.ones_like(args[1])))
    with pytest.raises(RuntimeError, match="recolor is not supported"):
        bwd(r, (x, scale, bgx))


def _passes_inputs(dev):
    from pcrender import synth
    cloud = synth.make_cloud("synth-THuman-256", seed=0, P=30000)
    g = synth.make_gaussians(cloud, profile="inference", seed=1)
    sf = cloud["scale_factor"]
    radius = np.sqrt(3) / sf * 6
    leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
    means, shs = leaf(g["means3D"]), leaf(g["shs"])
    opac, rots = leaf(g["opacities"]), leaf(g["rotations"])
    scales = leaf((g["scales"] / radius).astype(np.float32))
    normals = torch.nn.functional.normalize(_t(g["means3D"], dev) + 0.1, dim=-1).requires_grad_(True)
    return sf, means, opac, scales, rots, shs, normals


@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("bgv", [0.0, 1.0])
def test_train_passes_equals_literal_passes_under_autograd(gpu_device, with_normals, bgv):
    from pcrender import raster_passes as rp, camera
    dev = gpu_device
    sf, means, opac, scales, rots, shs, normals = _passes_inputs(dev)
    Hs = camera.circle_path(4, 0, 3, [90, 0])
    h = w = 96
    bg = torch.ones(3, device=dev) * bgv
    nrm = normals if with_normals else None
    weights = dict(xyz_w=1.0, rgb=0.01, hitmap=0.01, normal=10.0)
    rng = np.random.default_rng(3)
    R = {k: _t(rng.uniform(-1, 1, (1, 4, h, w, 3)).astype(np.float32), dev) for k in weights}
    leaves = dict(means3D=means, opacities=opac, scales=scales, rotations=rots, shs=shs, normals=normals)

    def run(fn):
        for t in leaves.values():
            t.grad = None
        out = fn(means, opac, scales, rots, shs, Hs, h, w, 45.0, bg, sf, normals=nrm, sh_degree=1, super_sample_rate=2)
        loss = sum(weights[k] * (out[k] * R[k]).sum() for k in weights if out[k] is not None)
        loss.backward()
        return out, {k: (None if t.grad is None else t.grad.detach().cpu().numpy().astype(np.float64)) for k, t in leaves.items()}

    out_t, g_t = run(rp.train_passes)
    out_l, g_l = run(rp.literal_passes)
    fused = rp.render_passes(means, opac, scales, rots, shs, Hs, h, w, 45.0, bg, sf, normals=nrm, sh_degree=1, super_sample_rate=2)
    for k in ("rgb", "xyz_w", "hitmap", "normal"):
        if fused[k] is None:
            assert out_t[k] is None
            continue
        assert torch.equal(out_t[k].detach(), fused[k]), k
    names = [k for k in leaves if g_l[k] is not None]
    assert ("normals" in names) == with_normals
    for k in names:
        assert g_t[k] is not None, k
    util.check_grads({k: g_t[k].reshape(g_t[k].shape[0], -1) for k in names},
                     {k: g_l[k].reshape(g_l[k].shape[0], -1) for k in names}, "train_passes", names=names)


def test_train_passes_falls_back_for_a_coloured_background(gpu_device):
    from pcrender import raster_passes as rp, camera
    dev = gpu_device
    sf, means, opac, scales, rots, shs, normals = _passes_inputs(dev)
    Hs = camera.circle_path(2, 0, 3, [90, 0])
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    a = rp.train_passes(means, opac, scales, rots, shs, Hs, 48, 48, 45.0, bg, sf, normals=normals)
    b = rp.literal_passes(means, opac, scales, rots, shs, Hs, 48, 48, 45.0, bg, sf, normals=normals)
    for k in a:
        assert torch.equal(a[k].detach(), b[k].detach()), k
    assert a["normal"].requires_grad


def test_full_size_split_channels_backward(gpu_device):
    """synth-THuman-800K at 1920 x 1080, 12 views, nx = 8 split layout, once, against the decomposition"""
    from diff_gaussian_rasterization import _native as N
    from pcrender import camera, synth
    dev = gpu_device
    cloud = synth.make_cloud("synth-THuman-800K", seed=0)
    g = synth.make_gaussians(cloud, profile="training", seed=1)
    W, H, V, nx = 1920, 1080, 12, 8
    views = camera.circle_views(12, fov_deg=45.0, width_px=W, height_px=H)
    args = _args(g, views, W, H, dev, bg=(0.0, 0.0, 0.0))
    P = g["means3D"].shape[0]
    x, scale, bgx, dense = _extra_inputs(P, V, nx, 2, dev, seed=12)
    rng = np.random.default_rng(6)
    dpix = _t(rng.uniform(-1, 1, (V, 3, H, W)).astype(np.float32), dev)
    dx = _t(rng.uniform(-1, 1, (V, nx, H, W)).astype(np.float32), dev)
    gp, gx, _ = _channels_bwd(N, args, x, scale, bgx, dpix, dx)
    go, gxo = _decomposition(N, args, V, P, nx, dense, scale, bgx, dpix, dx)
    _check(gp, go, gx, _fold(gxo, 2, V, P), "800K 1080p x 12 split")
