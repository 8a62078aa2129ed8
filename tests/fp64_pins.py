"""What the float64 pins of the backwards share (tests/test_gpu_channels_fp64.py, test_gpu_colour_fp64.py, the deterministic and
train-math tests, the sweeps): seeded inputs, the library call that returns records, the float64 and reference-build sums, and the
comparisons that hold one to the other.  Importable without torch, the built library or a device.

  SCALES / channel_inputs                    the extra channels' seeded values, view scales, backgrounds and dL
  channels_product / compare_batch           channels forward + backward with records; a batch held to float64
  CHECKED / check_channels_grads             a channels backward's gradients and dL/d values held to another's by util.check_grads
  flat64 / rel_err                           dL/d values as one float64 array; max |a - b| in units of max |b|
  ref_decomposition                          the same sums made of the reference build's float32 colour backwards
  synth_scenes / deep_stack_cloud / flipped_view / view_settings
                                             the clouds and cameras of the pins
  MATRIX_SCENES / CHAIN / scenes_dpix        the colour pin's edge scenes, chain leaves and seeded dL_dpix
  colour_fp64 / reference_sums               the float64 colour backward of a batch; the reference build's per-view sums
  colour_records_backward                    colour forward + backward: gradients, records, run tuple
  well_conditioned / ill_conditioned / colour_pin
                                             the colour backward held to float64
  recolor_setup / recolor / raw_forward      a need_backward recolor on a forward's arenas; gsr_forward_batch on given arenas"""
import numpy as np

import native_calls as NC
import util
from fp64_channels import _groups, channels_backward_fp64_scenes, fold_extra, with_colours

F = np.float32
SCALES = np.array([-2.0, -0.5, 0.0, 0.5, 3.0], F)
MATRIX_SCENES = ["random_aniso", "culled_mix", "opaque_early_stop", "deep_stack", "big_splats", "one_gaussian", "all_culled"]
CHAIN = ("dL_dmean3D", "dL_dscale", "dL_drot")
CHECKED = ("dL_dmean2D", "dL_dopacity", "dL_dmean3D", "dL_dscale", "dL_drot", "dL_dsh", "dL_dcolor")

# ---- the channels backward --------------------------------------------------------------------------------------------------------
def channel_inputs(P, V, nx, layout, seed, scales=None, H=None, W=None):
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


def channels_product(N, args, x, sc, bgx, dpix, dx, dev):
    """channels forward + backward: (per-Gaussian grads, dL/d values as a flat float64 array, records [V][P,16], run tuple)"""
    t = NC.to_device
    xt = tuple(t(a, dev) for a in x) if isinstance(x, tuple) else t(x, dev)
    st = None if sc is None else t(sc, dev)
    gp, gx, run = NC.channels_backward(N, args, xt, st, t(bgx, dev), t(dpix, dev), t(dx, dev))
    counts, color, radii, out_x, geom, binning, img = run
    P, V = args[1].shape[0], dpix.shape[0]
    rec = [N.grad_records(geom, P, view=v, n_views=V).cpu().numpy().astype(np.float64) if P else np.zeros((0, 16))
           for v in range(V)]
    return gp, gx.astype(np.float64), rec, run


def check_channels_grads(gp, go, gx, gxo, tag):
    util.check_grads({n: gp[n] for n in CHECKED}, {n: go[n] for n in CHECKED}, tag, names=CHECKED)
    util.check_grads({"dL_dextra": gx.reshape(-1, 1)}, {"dL_dextra": gxo.reshape(-1, 1)}, tag, names=("dL_dextra",))


def flat64(g):
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in g]) if isinstance(g, tuple) else np.asarray(g, np.float64)


def rel_err(a, b):
    """max |a - b| in units of max |b| (0 when both are zero)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.shape(a))
    m = np.abs(b).max() if b.size else 0.0
    d = np.abs(a - b).max() if b.size else 0.0
    return d / m if m > 0 else (0.0 if d == 0 else np.inf)


def ref_decomposition(ref, scenes, dense, sc, bgx, dpix, dx, images=None):
    """the same sums made of the reference build's float32 colour backwards: per view (mean2D [P,2], conic [P,3], opacity [P],
    colour [P,3], dL/d extra [P,nx]) and the eight per-Gaussian gradients summed over the views (dL_dcolor / dL_dsh: the colour
    run's).  images: an array [V, nx, H, W] that receives the forwards of the group runs (a group's three planes of out_color)"""
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


def compare_batch(N, oracle, scenes, x, dense, sc, bgx, dpix, dx, layout, dev, tag, conic_bar):
    want = channels_backward_fp64_scenes(oracle, scenes, dense, sc, bgx, dpix, dx)
    gp, gx, rec, run = channels_product(N, NC.scene_args(scenes, dev), x, sc, bgx, dpix, dx, dev)
    V = len(scenes)
    for v in range(V):
        w, r = want["views"][v], rec[v]
        util.check_grads({"opacity": r[:, 8:9], "colour": r[:, 5:8]}, {"opacity": w["opacity"][:, None], "colour": w["colour"]},
                         "%s view %d" % (tag, v), names=("opacity", "colour"))
        e2, ec = rel_err(r[:, 0:2], w["mean2D"]), rel_err(r[:, 2:5], w["conic"])
        # (observed: at most 5.4e-7 / 1.04e-6 of max|g| on these scenes)
        assert e2 <= conic_bar and ec <= conic_bar, (tag, v, e2, ec)
    gxo = flat64(fold_extra(np.stack([w["extra"] for w in want["views"]]), layout))
    util.check_grads({"dL_dextra": gx.reshape(-1, 1)}, {"dL_dextra": gxo.reshape(-1, 1)}, tag, names=("dL_dextra",))
    util.check_grads({"dL_dopacity": gp["dL_dopacity"], "dL_dcolor": gp["dL_dcolor"]},
                     {"dL_dopacity": want["grads"]["dL_dopacity"], "dL_dcolor": want["grads"]["dL_dcolor"]}, tag,
                     names=("dL_dopacity", "dL_dcolor"))
    return run


# ---- clouds and cameras -----------------------------------------------------------------------------------------------------------
def synth_scenes(V, P=40000, W=128, H=112, bg=(0.3, 0.3, 0.3)):
    g, views, W, H = NC.circle_scene(V, P=P, W=W, H=H)
    return g, views, W, H, [util.scene_from(g, v, W, H, bg=bg) for v in views]


def deep_stack_cloud(P, seed):
    """util's deep_stack cloud with P splats: one list per tile that no pixel terminates"""
    rng = np.random.default_rng(seed)
    W, H = 24, 16
    means = np.stack([rng.uniform(-0.25, 0.25, P), rng.uniform(-0.2, 0.2, P), rng.uniform(1.0, 3.0, P)], 1).astype(F)
    g = dict(means3D=means, scales=np.exp(rng.normal(np.log(0.08), 0.3, (P, 3))).astype(F),
             rotations=np.tile(np.array([1, 0, 0, 0], F), (P, 1)), opacities=rng.uniform(0.004, 0.0075, (P, 1)).astype(F),
             shs=(0.6 * rng.standard_normal((P, 4, 3))).astype(F), sh_degree=1)
    return g, W, H


def flipped_view(view):
    """the same camera turned round (x and z axes negated): it sees nothing of a cloud it faced"""
    import torch
    vm = np.asarray(view["viewmatrix"], np.float64).reshape(4, 4)
    pm = np.asarray(view["projmatrix"], np.float64).reshape(4, 4)
    proj = np.linalg.solve(vm, pm)                       # viewmatrix @ proj = projmatrix (row-vector convention)
    vm2 = vm * np.array([-1.0, 1.0, -1.0, 1.0])[None, :]
    out = dict(view)
    out["viewmatrix"] = torch.from_numpy((vm2).astype(F))
    out["projmatrix"] = torch.from_numpy((vm2 @ proj).astype(F))
    return out


def view_settings(views, W, H, bg, dev, sh_degree):
    import torch
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return [GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=v["tanfovx"], tanfovy=v["tanfovy"],
                                          bg=torch.as_tensor(np.asarray(bg, F), device=dev), scale_modifier=1.0,
                                          viewmatrix=v["viewmatrix"].to(dev), projmatrix=v["projmatrix"].to(dev), sh_degree=sh_degree,
                                          campos=v["campos"].to(dev), prefiltered=False, debug=False) for v in views]


# ---- the colour backward ----------------------------------------------------------------------------------------------------------
def scenes_dpix(scenes, seed):
    s = scenes[0]
    return np.random.default_rng(seed).uniform(-1, 1, (len(scenes), 3, s.H, s.W)).astype(F)


def colour_fp64(oracle, scenes, dpix):
    """the float64 colour backward of views `scenes` (one oracle Scene per view): per-view records and the summed chain"""
    V, P = len(scenes), scenes[0].P
    H, W = scenes[0].H, scenes[0].W
    return channels_backward_fp64_scenes(oracle, scenes, np.zeros((V, P, 0), F), None, np.zeros(0, F), dpix,
                                         np.zeros((V, 0, H, W), F))


def reference_sums(ref, scenes, dpix):
    """the same sums made of the reference build's float32 per-view backwards: per view (mean2D, conic), summed chain"""
    views, tot = [], {}
    for v, s in enumerate(scenes):
        _, g = ref.forward_backward(s, dpix[v])
        views.append(dict(mean2D=g["dL_dmean2D"][:, :2].astype(np.float64), conic=g["dL_dconic"][:, [0, 1, 3]].astype(np.float64)))
        for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dcov3D"):
            tot[k] = tot.get(k, 0.0) + g[k].astype(np.float64)
    return views, tot


def colour_records_backward(N, args, dpix, dev, run=None):
    """colour forward (need_backward) + gsr_backward_batch: (per-Gaussian grads, records [V][P,16] float64, run tuple)"""
    if run is None:
        run = N.rasterize_gaussians_batch(*args, need_backward=True)
    geom = run[3]
    g = N.rasterize_gaussians_backward_batch(*NC.colour_backward_args(args, run, NC.to_device(dpix, dev)))
    P, V = args[1].shape[0], dpix.shape[0]
    gp = {n: t.detach().cpu().numpy() for n, t in zip(util.GRAD_NAMES, g)}
    rec = [N.grad_records(geom, P, view=v, n_views=V).cpu().numpy().astype(np.float64) if P else np.zeros((0, 16)) for v in range(V)]
    return gp, rec, run


def well_conditioned(gp, rec, want, scenes, tag):
    """per-view colour / opacity records, dL_dcolor, dL_dopacity, dL_dsh, dL_dcov3D (precomputed covariance) against float64"""
    for v, (w, r) in enumerate(zip(want["views"], rec)):
        assert np.isfinite(r).all(), (tag, v)
        util.check_grads({"opacity": r[:, 8:9], "colour": r[:, 5:8]}, {"opacity": w["opacity"][:, None], "colour": w["colour"]},
                         "%s view %d" % (tag, v), names=("opacity", "colour"))
    gw = want["grads"]
    names = ["dL_dopacity", "dL_dcolor"] + (["dL_dsh"] if scenes[0].shs is not None else []) + \
        (["dL_dcov3D"] if scenes[0].cov3D_precomp is not None else [])
    exp = {"dL_dopacity": gw["dL_dopacity"], "dL_dcolor": gw["dL_dcolor"]}
    if "dL_dsh" in names:
        exp["dL_dsh"] = gw["dL_dsh"]
    if "dL_dcov3D" in names:
        exp["dL_dcov3D"] = gw["dL_dcov3D"]
    util.check_grads(gp, exp, tag, names=tuple(names))


def ill_conditioned(gp, rec, want, rv, rt, scenes):
    """(library error, reference build error) against float64 of mean2D, conic (per view, worst) and the chain (worst leaf)"""
    chain = CHAIN if scenes[0].scales is not None and scenes[0].cov3D_precomp is None else ("dL_dmean3D", "dL_dcov3D")
    lib = dict(mean2D=max(rel_err(r[:, 0:2], w["mean2D"]) for r, w in zip(rec, want["views"])),
               conic=max(rel_err(r[:, 2:5], w["conic"]) for r, w in zip(rec, want["views"])),
               chain=max(rel_err(gp[k], want["grads"][k]) for k in chain))
    ref = dict(mean2D=max(rel_err(r["mean2D"], w["mean2D"]) for r, w in zip(rv, want["views"])),
               conic=max(rel_err(r["conic"], w["conic"]) for r, w in zip(rv, want["views"])),
               chain=max(rel_err(rt[k], want["grads"][k]) for k in chain))
    return lib, ref


def colour_pin(N, oracle, ref, scenes, dpix, dev, tag, run=None, args=None, cache=None):
    """one colour backward against float64: well-conditioned outputs by check_grads; returns the ill-conditioned errors
    (None when nothing was drawn: then every record must be exactly zero).  cache: a dict that keeps the references of these
    scenes for further calls"""
    gp, rec, run = colour_records_backward(N, NC.scene_args(scenes, dev) if args is None else args, dpix, dev, run=run)
    cache = {} if cache is None else cache
    if "want" not in cache:
        cache["want"] = colour_fp64(oracle, scenes, dpix)
    want = cache["want"]
    well_conditioned(gp, rec, want, scenes, tag)
    if all(np.abs(w["conic"]).max(initial=0.0) == 0 for w in want["views"]):
        assert not any(r.any() for r in rec), tag
        return None, run
    if "ref" not in cache:
        cache["ref"] = reference_sums(ref, scenes, dpix)
    rv, rt = cache["ref"]
    return ill_conditioned(gp, rec, want, rv, rt, scenes), run


def recolor(N, args, run, colours=None, campos=None):
    """gsr_forward_recolor(need_backward = 1) on the arenas of `run`: with precomputed colours, or the arguments' SHs from campos"""
    return N.recolor(*NC.recolor_args(args, run, colours, campos), need_backward=True)


def recolor_setup(dev, V=2):
    g, views, W, H = NC.circle_scene(V, P=8000, W=96, H=80)
    g = dict(g)
    rng = np.random.default_rng(21)
    g["shs"] = (0.6 * rng.standard_normal(g["shs"].shape)).astype(F)      # view-dependent enough to change the clamp mask
    scenes = [util.scene_from(g, v, W, H, bg=(0.2, 0.2, 0.6)) for v in views]
    return g, scenes, NC.scene_args(scenes, dev)


def raw_forward(N, args, run, need_backward):
    """gsr_forward_batch with the given need_backward on the (full-size) arenas of `run`"""
    import ctypes as C
    import torch
    counts, color, radii, geom, binning, img = run[:6]
    V = len(counts)
    p, keep = N._params(*args, need_backward=need_backward)
    cnt = (C.c_int64 * V)()
    with torch.cuda.device(args[1].device):
        rc = N.lib.gsr_forward_batch(C.byref(p), V, geom.data_ptr(), geom.numel(), img.data_ptr(), img.numel(), binning.data_ptr(),
                                     binning.numel(), radii.data_ptr(), color.data_ptr(), cnt, 0,
                                     torch.cuda.current_stream(args[1].device).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, N.lib.gsr_last_error()
