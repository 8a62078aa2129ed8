"""The channels backward (k_render_backward<MODE, NX>, rasterize_views_channels) against the float64 reference of
tests/fp64_channels.py, in every moments mode and at the edges of the walk: partial tiles, culled splats, the T < 1e-4 stop,
lists longer than BWD_MAX_CHUNKS slices (the capped last slice, at both slice lengths), large off-centre splats (the adaptive
mode's per-batch switch), empty views.  The render-level records, dL/d extra and the per-Gaussian gradients are compared with
float64; the ill-conditioned ones (mean2D, conic and the chain through them) by their error against float64 relative to the error
of the same sums made of the reference build's float32 colour backwards."""
import numpy as np
import pytest
import torch

import util
from fp64_channels import channels_backward_fp64, channels_backward_fp64_scenes, extra_render_fp64, fold_extra
import test_gpu_channels_backward as CB

pytestmark = pytest.mark.gpu

F = np.float32
SCALES = np.array([-2.0, -0.5, 0.0, 0.5, 3.0], F)
MODES = (0, 1, 2)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _args(scenes, dev):
    """rasterize_gaussians_batch arguments for views of one cloud, given as oracle Scenes"""
    s = scenes[0]
    e = torch.empty(0)
    a = lambda x: e if x is None else _t(x, dev)  # noqa: E731
    vm = _t(np.stack([x.viewmatrix.reshape(4, 4) for x in scenes]), dev)
    pm = _t(np.stack([x.projmatrix.reshape(4, 4) for x in scenes]), dev)
    cp = _t(np.stack([x.campos.reshape(3) for x in scenes]), dev)
    return [a(s.bg), a(s.means3D), a(s.colors_precomp), a(s.opacities.reshape(-1, 1)), a(s.scales), a(s.rotations),
            float(s.scale_modifier), a(s.cov3D_precomp), vm, pm, s.tanfovx, s.tanfovy, s.H, s.W, a(s.shs),
            int(s.sh_degree) if s.shs is not None else 0, cp, False, False]


def _inputs(P, V, nx, layout, seed, scales=None, H=None, W=None):
    """values in `layout` (numpy), the dense [V][P][nx] values they stand for, view scales, bg_extra, dL_dpix, dL_dextra"""
    rng = np.random.default_rng(seed)
    if layout == 0:
        x = rng.normal(0, 1, (P, nx)).astype(F)
        dense = np.broadcast_to(x, (V, P, nx))
    elif layout == 1:
        x = rng.normal(0, 1, (V, P, nx)).astype(F)
        dense = x
    else:
        x = (rng.normal(0, 1, (P, 4)).astype(F), rng.normal(0, 1, (V, P, 4)).astype(F))
        dense = np.concatenate([np.broadcast_to(x[0], (V, P, 4)), x[1]], 2)
    sc = rng.choice(SCALES if scales is None else scales, (V, nx)).astype(F)
    bgx = rng.uniform(-1, 1, nx).astype(F)
    dpix = rng.uniform(-1, 1, (V, 3, H, W)).astype(F)
    dx = rng.uniform(-1, 1, (V, nx, H, W)).astype(F)
    return x, np.ascontiguousarray(dense), sc, bgx, dpix, dx


def _product(N, args, x, sc, bgx, dpix, dx, dev):
    """channels forward + backward: (per-Gaussian grads, dL/d values as a flat float64 array, records [V][P,16], run tuple)"""
    xt = tuple(_t(a, dev) for a in x) if isinstance(x, tuple) else _t(x, dev)
    st = None if sc is None else _t(sc, dev)
    gp, gx, run = CB._channels_bwd(N, args, xt, st, _t(bgx, dev), _t(dpix, dev), _t(dx, dev))
    counts, color, radii, out_x, geom, binning, img = run
    P, V = args[1].shape[0], dpix.shape[0]
    rec = [N.grad_records(geom, P, view=v, n_views=V).cpu().numpy().astype(np.float64) if P else np.zeros((0, 16))
           for v in range(V)]
    return gp, gx.astype(np.float64), rec, run


def _flat(g):
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in g]) if isinstance(g, tuple) else np.asarray(g, np.float64)


def _err(a, b):
    """max |a - b| in units of max |b| (0 when both are zero)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.shape(a))
    m = np.abs(b).max() if b.size else 0.0
    d = np.abs(a - b).max() if b.size else 0.0
    return d / m if m > 0 else (0.0 if d == 0 else np.inf)


def _ref_decomposition(ref, scenes, dense, sc, bgx, dpix, dx, images=None):
    """the same sums made of the reference build's float32 colour backwards: per view (mean2D [P,2], conic [P,3], opacity [P],
    colour [P,3], dL/d extra [P,nx]) and the eight per-Gaussian gradients summed over the views (dL_dcolor / dL_dsh: the colour
    run's).  images: an array [V, nx, H, W] that receives the forwards of the group runs (a group's three planes of out_color)"""
    from fp64_channels import _groups, with_colours
    V, P, nx = dense.shape
    views, tot = [], {}
    shared = ("dL_dmean2D", "dL_dopacity", "dL_dmean3D", "dL_dscale", "dL_drot", "dL_dcov3D")
    for v, s in enumerate(scenes):
        _, g = ref.forward_backward(s, dpix[v])
        m2, con = g["dL_dmean2D"][:, :2].astype(np.float64), g["dL_dconic"][:, [0, 1, 3]].astype(np.float64)
        op = g["dL_dopacity"].reshape(-1).astype(np.float64)
        for k in shared + ("dL_dcolor", "dL_dsh"):
            tot[k] = tot.get(k, 0.0) + g[k].astype(np.float64)
        gx = np.zeros((P, nx))
        for ks in _groups(nx):
            cols = np.zeros((P, 3), F)
            cols[:, :len(ks)] = dense[v][:, ks] * sc[v, ks]
            b3 = np.zeros(3, F)
            b3[:len(ks)] = bgx[ks]
            dl = np.zeros((3, s.H, s.W), F)
            dl[:len(ks)] = dx[v, ks]
            fw, gr = ref.forward_backward(with_colours(s, cols, b3), dl)
            if images is not None:
                images[v, ks] = fw["out_color"][:len(ks)]
            m2 = m2 + gr["dL_dmean2D"][:, :2]
            con = con + gr["dL_dconic"][:, [0, 1, 3]]
            op = op + gr["dL_dopacity"].reshape(-1)
            for k in shared:
                tot[k] = tot[k] + gr[k].astype(np.float64)
            gx[:, ks] = gr["dL_dcolor"][:, :len(ks)].astype(np.float64) * sc[v, ks]
        views.append(dict(mean2D=m2, conic=con, opacity=op, colour=g["dL_dcolor"].astype(np.float64), extra=gx))
    return views, tot


CHAIN = ("dL_dmean3D", "dL_dscale", "dL_drot")
MATRIX_SCENES = ["random_aniso", "culled_mix", "opaque_early_stop", "deep_stack", "big_splats", "one_gaussian", "all_culled"]


def test_kernel_matrix_against_float64(oracle, gpu_device):
    """every MODE x NX instantiation of the channels backward on the edge scenes, per-view values with non-unit scales"""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    ref = util.reference_build()
    err = {m: {k: [] for k in ("mean2D", "conic", "chain", "extra")} for m in MODES + ("ref",)}
    was = N.lib.gsr_set_backward_moments(-1)
    try:
        for name in MATRIX_SCENES:
            s = util.build_scene(name)
            P = s.P
            for nx in (4, 8):
                x, dense, sc, bgx, dpix, dx = _inputs(P, 1, nx, 1, seed=nx + len(name), scales=np.array([-2.0, -0.5, 0.5, 3.0], F),
                                                      H=s.H, W=s.W)
                want = channels_backward_fp64_scenes(oracle, [s], dense, sc, bgx, dpix, dx)
                w0 = want["views"][0]
                xa = extra_render_fp64(w0["fwd"], dense[0], bgx, dx[0], scale=sc[0])
                assert np.abs(xa["grad"] - w0["extra"]).max() <= 1e-9 * max(np.abs(w0["extra"]).max(), 1e-30), name
                rv, rt = _ref_decomposition(ref, [s], dense, sc, bgx, dpix, dx)
                if np.abs(w0["conic"]).max() > 0:
                    err["ref"]["mean2D"].append(_err(rv[0]["mean2D"], w0["mean2D"]))
                    err["ref"]["conic"].append(_err(rv[0]["conic"], w0["conic"]))
                    err["ref"]["chain"].append(max(_err(rt[k], want["grads"][k]) for k in CHAIN))
                    err["ref"]["extra"].append(_err(rv[0]["extra"], xa["grad"]))
                for mode in MODES:
                    assert N.lib.gsr_set_backward_moments(mode) == mode
                    tag = "%s nx=%d mode=%d" % (name, nx, mode)
                    gp, gx, rec, _ = _product(N, _args([s], dev), x, sc, bgx, dpix, dx, dev)
                    r = rec[0]
                    assert np.isfinite(r).all() and np.isfinite(gx).all(), tag
                    util.check_grads({"opacity": r[:, 8:9], "colour": r[:, 5:8], "dL_dextra": gx.reshape(-1, 1)},
                                     {"opacity": w0["opacity"][:, None], "colour": w0["colour"], "dL_dextra": xa["grad"].reshape(-1, 1)},
                                     tag, names=("opacity", "colour", "dL_dextra"))
                    util.check_grads({"dL_dopacity": gp["dL_dopacity"]}, {"dL_dopacity": want["grads"]["dL_dopacity"]}, tag,
                                     names=("dL_dopacity",))
                    if np.abs(w0["conic"]).max() == 0:
                        # nothing drawn: every sum is exactly zero
                        assert not r.any() and not gx.any(), tag
                        continue
                    err[mode]["mean2D"].append(_err(r[:, 0:2], w0["mean2D"]))
                    err[mode]["conic"].append(_err(r[:, 2:5], w0["conic"]))
                    err[mode]["chain"].append(max(_err(gp[k], want["grads"][k]) for k in CHAIN))
                    err[mode]["extra"].append(_err(gx, xa["grad"]))
    finally:
        N.lib.gsr_set_backward_moments(was)
    med = {m: {k: float(np.median(v)) for k, v in e.items()} for m, e in err.items()}
    for m in MODES:
        print("channels backward, moments mode %d: median error against float64 / the reference build's: %s" % (
            m, ", ".join("%s %.2fx" % (k, med[m][k] / med["ref"][k]) for k in ("mean2D", "conic", "chain", "extra"))))
    print("reference build medians: %s" % med["ref"])
    # observed (MI355X, two runs, 12 cases with hits) mean2D / conic / chain / dL_dextra: mode 0 1.37-1.38x / 2.7-3.0x / 4.8-4.9x /
    # 0.9-1.0x, mode 1 0.94-1.05x / 1.9-2.0x / 1.21x / 1.02-1.03x, mode 2 (the default) 1.14-1.21x / 1.9-2.1x / 1.8x / 1.02-1.10x;
    # the colour backward's mode 2: 1.33x / 2.1x (profiles/r06_bwd_accuracy.txt)
    bars = {0: dict(mean2D=2.0, conic=4.5, chain=7.5, extra=1.5), 1: dict(mean2D=1.5, conic=3.0, chain=2.0, extra=1.5),
            2: dict(mean2D=1.8, conic=3.0, chain=2.7, extra=1.5)}
    for m in MODES:
        for k, c in bars[m].items():
            assert med[m][k] <= c * med["ref"][k], (m, k, med[m][k], med["ref"][k])


def _synth(V, P=40000, W=128, H=112, bg=(0.3, 0.3, 0.3)):
    g, views, W, H = CB._scene(V, P=P, W=W, H=H)
    return g, views, W, H, [util.scene_from(g, v, W, H, bg=bg) for v in views]


def _longest(N, run, P, W, H, V):
    counts, _, _, _, geom, binning, img = run
    return CB._long_lists(N, geom, binning, img, counts, P, W, H, V)


def _compare_batch(N, oracle, scenes, x, dense, sc, bgx, dpix, dx, layout, dev, tag, conic_bar):
    want = channels_backward_fp64_scenes(oracle, scenes, dense, sc, bgx, dpix, dx)
    gp, gx, rec, run = _product(N, _args(scenes, dev), x, sc, bgx, dpix, dx, dev)
    V = len(scenes)
    for v in range(V):
        w, r = want["views"][v], rec[v]
        util.check_grads({"opacity": r[:, 8:9], "colour": r[:, 5:8]}, {"opacity": w["opacity"][:, None], "colour": w["colour"]},
                         "%s view %d" % (tag, v), names=("opacity", "colour"))
        e2, ec = _err(r[:, 0:2], w["mean2D"]), _err(r[:, 2:5], w["conic"])
        # (observed: at most 5.4e-7 / 1.04e-6 of max|g| on these scenes)
        assert e2 <= conic_bar and ec <= conic_bar, (tag, v, e2, ec)
    gxo = _flat(fold_extra(np.stack([w["extra"] for w in want["views"]]), layout))
    util.check_grads({"dL_dextra": gx.reshape(-1, 1)}, {"dL_dextra": gxo.reshape(-1, 1)}, tag, names=("dL_dextra",))
    util.check_grads({"dL_dopacity": gp["dL_dopacity"], "dL_dcolor": gp["dL_dcolor"]},
                     {"dL_dopacity": want["grads"]["dL_dopacity"], "dL_dcolor": want["grads"]["dL_dcolor"]}, tag,
                     names=("dL_dopacity", "dL_dcolor"))
    return run


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_batch_of_three_views_with_long_lists(oracle, gpu_device, layout):
    """V = 3: 1024-entry slices starting at saved boundaries; scales drawn from {-2, -0.5, 0, 0.5, 3}"""
    from diff_gaussian_rasterization import _native as N
    g, views, W, H, scenes = _synth(3)
    P = scenes[0].P
    x, dense, sc, bgx, dpix, dx = _inputs(P, 3, 8, layout, seed=20 + layout, H=H, W=W)
    run = _compare_batch(N, oracle, scenes, x, dense, sc, bgx, dpix, dx, layout, gpu_device, "synth V=3 layout=%d" % layout, 1e-5)
    assert _longest(N, run, P, W, H, 3) > 2048


def test_no_view_scale(oracle, gpu_device):
    """extra_view_scale = None (the kernels' extra_scale == nullptr branch), V = 2 shared values"""
    from diff_gaussian_rasterization import _native as N
    g, views, W, H, scenes = _synth(2, P=20000, W=96, H=80)
    P = scenes[0].P
    x, dense, _, bgx, dpix, dx = _inputs(P, 2, 4, 0, seed=31, H=H, W=W)
    # the reference with all-one scales is the same render
    _compare_batch(N, oracle, scenes, x, dense, None, bgx, dpix, dx, 0, gpu_device, "no view scale", 1e-5)


def _deep_stack(P, seed):
    """util's deep_stack cloud with P splats: one list per tile that no pixel terminates"""
    rng = np.random.default_rng(seed)
    W, H = 24, 16
    means = np.stack([rng.uniform(-0.25, 0.25, P), rng.uniform(-0.2, 0.2, P), rng.uniform(1.0, 3.0, P)], 1).astype(F)
    g = dict(means3D=means, scales=np.exp(rng.normal(np.log(0.08), 0.3, (P, 3))).astype(F),
             rotations=np.tile(np.array([1, 0, 0, 0], F), (P, 1)), opacities=rng.uniform(0.004, 0.0075, (P, 1)).astype(F),
             shs=(0.6 * rng.standard_normal((P, 4, 3))).astype(F), sh_degree=1)
    return g, W, H


@pytest.mark.parametrize("V,P", [(1, 20000), (2, 36000)])
def test_capped_last_slice(oracle, gpu_device, V, P):
    """lists longer than BWD_MAX_CHUNKS slices: the last slice takes the rest (512-entry slices at V = 1, 1024 at V = 2)"""
    from diff_gaussian_rasterization import _native as N
    g, W, H = _deep_stack(P, 13)
    cam = util.identity_camera(W, H)
    scenes = [util.scene_from(g, cam, W, H, bg=(0.2, 0.3, 0.4)) for _ in range(V)]
    x, dense, sc, bgx, dpix, dx = _inputs(P, V, 4, 1, seed=40 + V, H=H, W=W)
    run = _compare_batch(N, oracle, scenes, x, dense, sc, bgx, dpix, dx, 1, gpu_device, "deep stack V=%d" % V, 1e-5)
    shift = 9 if V == 1 else 10
    assert _longest(N, run, P, W, H, V) > 32 << shift, "the list no longer reaches the capped last slice"


def _flip(view):
    """the same camera turned round (x and z axes negated): it sees nothing of a cloud it faced"""
    vm = np.asarray(view["viewmatrix"], np.float64).reshape(4, 4)
    pm = np.asarray(view["projmatrix"], np.float64).reshape(4, 4)
    proj = np.linalg.solve(vm, pm)                       # viewmatrix @ proj = projmatrix (row-vector convention)
    vm2 = vm * np.array([-1.0, 1.0, -1.0, 1.0])[None, :]
    out = dict(view)
    out["viewmatrix"] = torch.from_numpy((vm2).astype(F))
    out["projmatrix"] = torch.from_numpy((vm2 @ proj).astype(F))
    return out


def test_empty_views(oracle, gpu_device):
    """P = 0, a scene with everything culled, and a V = 3 batch whose middle camera faces away: no error, finite results,
    exactly zero dL/d extra where nothing was hit"""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    # all culled
    s = util.build_scene("all_culled")
    x, dense, sc, bgx, dpix, dx = _inputs(s.P, 1, 8, 1, seed=50, H=s.H, W=s.W)
    gp, gx, rec, run = _product(N, _args([s], dev), x, sc, bgx, dpix, dx, dev)
    assert not gx.any() and not rec[0].any() and all(np.isfinite(a).all() for a in gp.values())
    assert torch.equal(run[3][0], _t(np.broadcast_to(bgx[:, None, None], (8, s.H, s.W)), dev))
    # P = 0
    s0 = util.Scene(W=32, H=24, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=s.bg, means3D=np.zeros((0, 3), F),
                    opacities=np.zeros((0, 1), F), viewmatrix=s.viewmatrix, projmatrix=s.projmatrix, campos=s.campos,
                    colors_precomp=np.zeros((0, 3), F), scales=np.zeros((0, 3), F), rotations=np.zeros((0, 4), F))
    x, dense, sc, bgx, dpix, dx = _inputs(0, 2, 4, 1, seed=51, H=24, W=32)
    gp, gx, rec, run = _product(N, _args([s0, s0], dev), x, sc, bgx, dpix, dx, dev)
    assert gx.size == 0 and all(a.size == 0 or np.isfinite(a).all() for a in gp.values())
    # the middle view of three sees nothing
    g, views, W, H = CB._scene(3, P=12000, W=96, H=80)
    views = [views[0], _flip(views[1]), views[2]]
    scenes = [util.scene_from(g, v, W, H, bg=(0.1, 0.2, 0.3)) for v in views]
    P = scenes[0].P
    x, dense, sc, bgx, dpix, dx = _inputs(P, 3, 8, 1, seed=52, H=H, W=W)
    run = _compare_batch(N, oracle, scenes, x, dense, sc, bgx, dpix, dx, 1, dev, "middle view empty", 1e-5)
    counts, color, radii, out_x = run[:4]
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
    gp, gx, rec, _ = _product(N, _args(scenes, dev), x, sc, bgx, dpix, dx, dev)
    gx = gx.reshape(3, P, 8)
    assert not gx[1].any() and gx[0].any() and gx[2].any()
    assert not rec[1].any()
    assert torch.equal(out_x[1], _t(np.broadcast_to(bgx[:, None, None], (8, H, W)), dev))


# ------------------------------------------------------------------------------------------------ the autograd function
AUTOGRAD = [  # nx, per view, colours (SH / precomputed), covariance (scale + rotation / precomputed)
    (1, False, "sh", "sr"), (2, True, "colors", "cov"), (3, False, "colors", "sr"), (5, True, "sh", "cov"), (6, False, "sh", "cov"),
    (7, True, "colors", "sr")]


def _settings(views, W, H, bg, dev, sh_degree):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return [GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=v["tanfovx"], tanfovy=v["tanfovy"],
                                          bg=torch.as_tensor(np.asarray(bg, F), device=dev), scale_modifier=1.0,
                                          viewmatrix=v["viewmatrix"].to(dev), projmatrix=v["projmatrix"].to(dev), sh_degree=sh_degree,
                                          campos=v["campos"].to(dev), prefiltered=False, debug=False) for v in views]


@pytest.mark.parametrize("nx,per_view,col,cov", AUTOGRAD)
def test_rasterize_views_channels_autograd(oracle, gpu_device, nx, per_view, col, cov):
    from diff_gaussian_rasterization import rasterize_views_channels
    dev = gpu_device
    V = 2
    g, views, W, H = CB._scene(V, P=8000, W=96, H=80)
    P = g["means3D"].shape[0]
    rng = np.random.default_rng(nx)
    g = dict(g)
    g["colors_precomp"] = rng.uniform(0, 1, (P, 3)).astype(F)
    bg = (0.0, 0.0, 0.0)
    x = rng.normal(0, 1, ((V, P, nx) if per_view else (P, nx))).astype(F)
    dense = x if per_view else np.broadcast_to(x, (V, P, nx))
    sc = rng.choice(SCALES, (V, nx)).astype(F)
    bgx = rng.uniform(-1, 1, nx).astype(F)
    dpix = rng.uniform(-1, 1, (V, 3, H, W)).astype(F)
    dx = rng.uniform(-1, 1, (V, nx, H, W)).astype(F)
    leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
    L = dict(means3D=leaf(g["means3D"]), opacities=leaf(g["opacities"]), extra=leaf(x))
    L["means2D"] = torch.zeros((P, 3), device=dev, requires_grad=True)
    if col == "sh":
        L["shs"] = leaf(g["shs"])
    else:
        L["colors_precomp"] = leaf(g["colors_precomp"])
    if cov == "sr":
        L["scales"], L["rotations"] = leaf(g["scales"]), leaf(g["rotations"])
    else:
        L["cov3D_precomp"] = leaf(util.cov3d_from(g["scales"], g["rotations"]))
    sts = _settings(views, W, H, bg, dev, g["sh_degree"])
    kw = {k: v for k, v in L.items() if k not in ("means3D", "means2D", "opacities", "extra")}
    color, radii, ex = rasterize_views_channels(L["means3D"], L["means2D"], L["opacities"], sts, L["extra"], _t(bgx, dev),
                                                extra_view_scale=_t(sc, dev), **kw)
    assert tuple(ex.shape) == (V, nx, H, W)
    ((color * _t(dpix, dev)).sum() + (ex * _t(dx, dev)).sum()).backward()
    assert tuple(L["extra"].grad.shape) == tuple(x.shape)
    # the same call with eight channels, the added ones explicit zeros: the same images, bit for bit
    n8 = 8
    pad = lambda a, v: torch.cat([a, torch.full(tuple(a.shape[:-1]) + (n8 - nx,), v, device=dev)], -1)  # noqa: E731
    with torch.no_grad():
        c8, _, e8 = rasterize_views_channels(L["means3D"], L["means2D"], L["opacities"], sts, pad(L["extra"], 0.0),
                                             pad(_t(bgx, dev), 0.0), extra_view_scale=pad(_t(sc, dev), 1.0), **kw)
    assert torch.equal(c8, color) and torch.equal(e8[:, :nx], ex)
    # float64 reference
    scenes = [util.scene_from(g, v, W, H, bg=bg, mode=col, use_cov3d=(cov == "cov")) for v in views]
    want = channels_backward_fp64(oracle, g, views, W, H, dense, sc, bgx, dpix, dx, bg=bg, mode=col, use_cov3d=(cov == "cov"))
    gw = want["grads"]
    gx = fold_extra(np.stack([w["extra"] for w in want["views"]]), int(per_view))
    tag = "nx=%d per_view=%s %s %s" % (nx, per_view, col, cov)
    got = {"extra": L["extra"].grad, "opacities": L["opacities"].grad}
    exp = {"extra": gx, "opacities": gw["dL_dopacity"]}
    if col == "sh":
        got["shs"], exp["shs"] = L["shs"].grad, gw["dL_dsh"]
    else:
        got["colors_precomp"], exp["colors_precomp"] = L["colors_precomp"].grad, gw["dL_dcolor"]
    got = {k: v.detach().cpu().numpy().reshape(-1, 1) if k == "extra" else v.detach().cpu().numpy().reshape(P, -1) for k, v in got.items()}
    exp = {k: np.asarray(v).reshape(-1, 1) if k == "extra" else np.asarray(v).reshape(P, -1) for k, v in exp.items()}
    util.check_grads(got, exp, tag, names=tuple(got))
    # the ill-conditioned chain: against float64, no further off than the reference build's decomposition of the same sums
    rv, rt = _ref_decomposition(util.reference_build(), scenes, np.ascontiguousarray(dense), sc, bgx, dpix, dx)
    chain = {"means3D": "dL_dmean3D"}
    chain.update({"scales": "dL_dscale", "rotations": "dL_drot"} if cov == "sr" else {"cov3D_precomp": "dL_dcov3D"})
    for leaf_name, k in chain.items():
        a = L[leaf_name].grad.detach().cpu().numpy()
        e_lib, e_ref = _err(a, gw[k]), _err(rt[k], gw[k])
        # (observed: 0.9x - 3.3x, single cases of 8000 splats, errors of ~1e-6 of max|g|)
        assert e_lib <= 6.0 * e_ref, (tag, leaf_name, e_lib, e_ref)
    m2 = L["means2D"].grad.detach().cpu().numpy()
    assert _err(m2[:, :2], gw["dL_dmean2D"][:, :2]) <= 4.0 * max(_err(sum(r["mean2D"] for r in rv), gw["dL_dmean2D"][:, :2]), 1e-6), tag
