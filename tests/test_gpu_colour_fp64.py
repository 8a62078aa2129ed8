"""The colour backward (k_render_backward<MODE, 0> + k_preprocess_backward, gsr_backward_batch) against a float64 reference, in
every moments mode and at the edges of the walk: partial tiles, culled splats, the T < 1e-4 stop, lists longer than BWD_MAX_CHUNKS
slices (the capped last slice, at both slice lengths), empty views, batches whose views differ in visibility and SH clamp mask,
the benchmark's 12 views, and backwards after gsr_forward_recolor.  Also the misuse gsr_backward_batch refuses (gsr.h).

The reference is the oracle's float64 render backward per view plus tests/fp64_backward.py's per-Gaussian chain, run per view with
that view's radii, clamp mask and campos and summed over the views (fp64_channels.channels_backward_fp64_scenes with no extra
channel).  The render-level records and the well-conditioned gradients are held to util.check_grads against it; the ill-conditioned
ones (mean2D, conic and the chain through them) by their error against float64 relative to the error of the same sums made of the
reference build's float32 per-view backwards."""
import numpy as np
import pytest
import torch

import util
from fp64_channels import with_colours
from fp64_pins import (MATRIX_SCENES, colour_fp64 as _fp64, colour_pin as _pin, colour_records_backward as _backward,
                       deep_stack_cloud as _deep_stack, flipped_view as _flip, ill_conditioned as _ill_conditioned, raw_forward as _raw_forward,
                       recolor as _recolor, recolor_setup as _recolor_setup, reference_sums as _ref, rel_err as _err, scenes_dpix as _dpix,
                       synth_scenes as _synth, well_conditioned as _well_conditioned)
from native_calls import circle_scene as _scene, longest_list as _long_lists, moments, scene_args as _args, to_device as _t

pytestmark = pytest.mark.gpu

F = np.float32
MODES = (0, 1, 2)
# caps on the median error against float64 in units of the reference build's, per (moments mode, V), with a margin of 1.4x or more
# over the ratios observed on an MI355X in two runs (mean2D / conic / chain; float atomics make them vary from run to run).
# V = 1: mode 0 2.10-2.25x / 2.11-2.30x / 4.22-5.46x, mode 1 1.42-1.52x / 1.18-1.29x / 1.40x, mode 2 1.46-1.56x / 1.17-1.18x / 1.39-1.40x.
# V = 3 (one case, the dense synthetic cloud): mode 0 2.81x / 3.27x / 4.91x, modes 1 and 2 2.85x / 2.07x / 1.99x -- the cloud rather
# than the view count: its first view alone at V = 1 gives 2.39x / 3.68x / 4.43x and 2.41x / 2.80x / 3.45x (printed, not capped)
BARS = {(0, 1): dict(mean2D=3.4, conic=3.5, chain=8.0), (1, 1): dict(mean2D=2.4, conic=2.0, chain=2.1),
        (2, 1): dict(mean2D=2.4, conic=2.0, chain=2.1), (0, 3): dict(mean2D=4.3, conic=5.0, chain=7.4),
        (1, 3): dict(mean2D=4.3, conic=3.1, chain=3.0), (2, 3): dict(mean2D=4.3, conic=3.1, chain=3.0)}


def test_moments_modes_against_float64(oracle, gpu_device):
    """every moments mode on the edge scenes (V = 1) and on a 3-view batch of one cloud"""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    ref = util.reference_build()
    g, views, W, H, batch = _synth(3, P=12000, W=96, H=80)
    cases = [(name, [util.build_scene(name)]) for name in MATRIX_SCENES] + [("synth view 0", batch[:1]), ("synth V=3", batch)]
    err = {(m, v): {k: [] for k in ("mean2D", "conic", "chain")} for m in MODES + ("ref",) for v in (1, 3)}
    with moments(None):
        for name, scenes in cases:
            dpix = _dpix(scenes, 7 + len(name))
            V = len(scenes)
            cache = {}
            for mode in MODES:
                assert N.lib.gsr_set_backward_moments(mode) == mode
                e, _ = _pin(N, oracle, ref, scenes, dpix, dev, "%s mode=%d" % (name, mode), cache=cache)
                if e is None:
                    continue
                lib, r = e
                if name.startswith("synth"):
                    print("%s, moments mode %d: error against float64 / the reference build's: %s" % (
                        name, mode, ", ".join("%s %.2fx" % (k, lib[k] / r[k]) for k in ("mean2D", "conic", "chain"))))
                if name == "synth view 0":
                    continue   # (printed only: the V = 3 case's cloud seen at V = 1, for comparison; not part of the medians)
                for k in lib:
                    err[(mode, V)][k].append(lib[k])
                    if mode == MODES[0]:
                        err[("ref", V)][k].append(r[k])
    med = {key: {k: float(np.median(a)) for k, a in e.items()} for key, e in err.items()}
    for V in (1, 3):
        for m in MODES:
            print("colour backward, moments mode %d, V = %d: median error against float64 / the reference build's: %s" % (
                m, V, ", ".join("%s %.2fx" % (k, med[(m, V)][k] / med[("ref", V)][k]) for k in ("mean2D", "conic", "chain"))))
        print("reference build medians, V = %d: %s" % (V, med[("ref", V)]))
    for V in (1, 3):
        for m in MODES:
            for k, c in BARS[(m, V)].items():
                assert med[(m, V)][k] <= c * med[("ref", V)][k], (m, V, k, med[(m, V)][k], med[("ref", V)][k])


def _unit(q):
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


def _views_that_differ(P=4000, W=112, H=96, seed=3):
    """an SH degree-3 cloud and three cameras: the second stands inside the cloud (part of it behind the camera or closer than the
    near plane), the third is shifted sideways (part of it outside the frustum); strong view-dependent SH make the clamp mask of
    many Gaussians differ between the views"""
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-0.8, 0.8, P), rng.uniform(-0.6, 0.6, P), rng.uniform(1.5, 4.0, P)], 1).astype(F)
    g = dict(means3D=means, scales=np.exp(rng.normal(np.log(0.03), 0.4, (P, 3))).astype(F),
             rotations=_unit(rng.normal(0, 1, (P, 4))), opacities=rng.uniform(0.05, 0.9, (P, 1)).astype(F),
             shs=(0.5 * rng.standard_normal((P, 16, 3))).astype(F), sh_degree=3)
    cams = []
    for t in ((0.0, 0.0, 0.0), (0.0, 0.0, 2.5), (0.9, 0.3, 0.5)):
        c2w = np.eye(4, dtype=F)
        c2w[:3, 3] = t
        cams.append(util._view_arrays(c2w, W, H, 60.0))
    return g, cams, W, H


def test_batch_views_differ_in_visibility_and_clamp_mask(oracle, gpu_device):
    """V = 3 with per-view differences in what k_preprocess_backward reads per view: campos, clamp mask and radii"""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    g, cams, W, H = _views_that_differ()
    scenes = [util.scene_from(g, c, W, H, bg=(0.1, 0.4, 0.7)) for c in cams]
    P = scenes[0].P
    fwd = [oracle.forward(s) for s in scenes]
    vis = [f["radii"] > 0 for f in fwd]
    z1 = g["means3D"].astype(np.float64) @ scenes[1].viewmatrix.reshape(4, 4)[:3, 2] + scenes[1].viewmatrix.reshape(4, 4)[3, 2]
    behind = vis[0] & (z1 <= 0.2)
    out_of_frame = vis[0] & ~vis[2]
    clamp_diff = (fwd[0]["clamped"] != fwd[1]["clamped"]).any(1) & vis[0] & vis[1]
    clamp_diff2 = (fwd[0]["clamped"] != fwd[2]["clamped"]).any(1) & vis[0] & vis[2]
    print("visible in view 0 and behind camera 1: %d; out of view 2's frame: %d; clamp mask differs (views 0/1, 0/2): %d / %d of %d" % (
        behind.sum(), out_of_frame.sum(), clamp_diff.sum(), clamp_diff2.sum(), P))
    assert behind.sum() >= 200 and out_of_frame.sum() >= 200, "the views no longer differ in visibility"
    assert clamp_diff.sum() >= 200 and clamp_diff2.sum() >= 200, "the views no longer differ in their SH clamp masks"
    ref = util.reference_build()
    dpix = _dpix(scenes, 11)
    e, _ = _pin(N, oracle, ref, scenes, dpix, dev, "views that differ")
    lib, r = e
    # (single case: the bars of the autograd tests, test_gpu_channels_fp64)
    assert lib["chain"] <= 6.0 * r["chain"] and lib["mean2D"] <= 4.0 * max(r["mean2D"], 1e-6), (lib, r)


@pytest.mark.parametrize("V,P", [(1, 20000), (2, 36000)])
def test_capped_last_slice(oracle, gpu_device, V, P):
    """lists longer than BWD_MAX_CHUNKS slices: the last slice takes the rest (512-entry slices at V = 1, 1024 at V = 2)"""
    from diff_gaussian_rasterization import _native as N
    g, W, H = _deep_stack(P, 17)
    cam = util.identity_camera(W, H)
    scenes = [util.scene_from(g, cam, W, H, bg=(0.2, 0.3, 0.4)) for _ in range(V)]
    dpix = _dpix(scenes, 60 + V)
    gp, rec, run = _backward(N, _args(scenes, gpu_device), dpix, gpu_device)
    want = _fp64(oracle, scenes, dpix)
    _well_conditioned(gp, rec, want, scenes, "deep stack V=%d" % V)
    for v in range(V):
        e2, ec = _err(rec[v][:, 0:2], want["views"][v]["mean2D"]), _err(rec[v][:, 2:5], want["views"][v]["conic"])
        # (the channels kernels' bar on these lists, test_gpu_channels_fp64)
        assert e2 <= 1e-5 and ec <= 1e-5, (V, v, e2, ec)
    shift = 9 if V == 1 else 10
    counts, _, _, geom, binning, img = run
    assert _long_lists(N, geom, binning, img, counts, P, W, H, V) > 32 << shift, "the list no longer reaches the capped last slice"


def test_empty_middle_view(oracle, gpu_device):
    """V = 3 whose middle camera faces away: its records are exactly zero, the gradients come from the other two views"""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    g, views, W, H = _scene(3, P=12000, W=96, H=80)
    views = [views[0], _flip(views[1]), views[2]]
    scenes = [util.scene_from(g, v, W, H, bg=(0.1, 0.2, 0.3)) for v in views]
    dpix = _dpix(scenes, 12)
    ref = util.reference_build()
    e, run = _pin(N, oracle, ref, scenes, dpix, dev, "middle view empty")
    counts = run[0]
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
    gp, rec, _ = _backward(N, _args(scenes, dev), dpix, dev, run=run)
    assert not rec[1].any() and rec[0].any() and rec[2].any()
    # the two other views alone give the same per-Gaussian gradients
    two = [scenes[0], scenes[2]]
    gp2, _, _ = _backward(N, _args(two, dev), dpix[[0, 2]], dev)
    util.check_grads(gp, gp2, "middle view empty vs the two other views", names=("dL_dopacity", "dL_dcolor", "dL_dsh"))
    lib, r = e
    assert lib["chain"] <= 6.0 * r["chain"] and lib["mean2D"] <= 4.0 * max(r["mean2D"], 1e-6), (lib, r)


def test_twelve_views(oracle, gpu_device):
    """the benchmark's view count on a small image: per-view strides of every arena at V = 12"""
    from diff_gaussian_rasterization import _native as N
    g, views, W, H = _scene(12, P=6000, W=64, H=48)
    scenes = [util.scene_from(g, v, W, H, bg=(0.3, 0.3, 0.3)) for v in views]
    e, _ = _pin(N, oracle, util.reference_build(), scenes, _dpix(scenes, 13), gpu_device, "V=12")
    lib, r = e
    assert lib["chain"] <= 6.0 * r["chain"] and lib["mean2D"] <= 4.0 * max(r["mean2D"], 1e-6), (lib, r)


def test_precomputed_covariance_and_colours(oracle, gpu_device):
    """V = 2 with cov3D_precomp and colors_precomp: dL_dcov3D and dL_dcolor are outputs of their own"""
    from diff_gaussian_rasterization import _native as N
    g, views, W, H = _scene(2, P=8000, W=96, H=80)
    g = dict(g)
    g["colors_precomp"] = np.random.default_rng(4).uniform(0, 1, (g["means3D"].shape[0], 3)).astype(F)
    scenes = [util.scene_from(g, v, W, H, bg=(0.5, 0.2, 0.1), mode="colors", use_cov3d=True) for v in views]
    e, _ = _pin(N, oracle, util.reference_build(), scenes, _dpix(scenes, 14), gpu_device, "cov3D + colours")
    lib, r = e
    assert lib["chain"] <= 6.0 * r["chain"], (lib, r)


# ------------------------------------------------------------------------------------------------ backward after a recolor
def _moved(s, campos):
    """the Scene s seen from the same camera, its SH evaluated from another camera position"""
    return util.Scene(W=s.W, H=s.H, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=s.bg, means3D=s.means3D, opacities=s.opacities,
                      viewmatrix=s.viewmatrix, projmatrix=s.projmatrix, campos=np.asarray(campos, F), shs=s.shs, sh_degree=s.sh_degree,
                      scales=s.scales, rotations=s.rotations, scale_modifier=s.scale_modifier)


def _pin_recolor(N, oracle, scenes, args, run, dpix, dev, tag):
    gp, rec, _ = _backward(N, args, dpix, dev, run=run)
    want = _fp64(oracle, scenes, dpix)
    _well_conditioned(gp, rec, want, scenes, tag)
    rv, rt = _ref(util.reference_build(), scenes, dpix)
    lib, r = _ill_conditioned(gp, rec, want, rv, rt, scenes)
    assert lib["chain"] <= 6.0 * r["chain"] and lib["mean2D"] <= 4.0 * max(r["mean2D"], 1e-6), (tag, lib, r)


@pytest.mark.parametrize("kind", ["sh_other_campos", "colours_shared", "colours_per_view", "twice"])
def test_backward_after_recolor(oracle, gpu_device, kind):
    """need_backward forward, gsr_forward_recolor(need_backward = 1), gsr_backward_batch: the gradients of the LAST colours rendered"""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    g, scenes, args = _recolor_setup(dev)
    V, P = len(scenes), scenes[0].P
    run = N.rasterize_gaussians_batch(*args, need_backward=True)
    rng = np.random.default_rng(30)
    dpix = _dpix(scenes, 31)
    args = list(args)
    if kind in ("sh_other_campos", "twice"):
        if kind == "twice":
            # a first recolor with other colours: the backward must not see them
            _recolor(N, args, run, colours=_t(rng.uniform(0, 1, (P, 3)).astype(F), dev))
        cp = np.stack([s.campos + np.array([0.9, -0.6, 0.7], F) * (1 + v) for v, s in enumerate(scenes)]).astype(F)
        out = _recolor(N, args, run, campos=_t(cp, dev))
        moved = [_moved(s, cp[v]) for v, s in enumerate(scenes)]
        # the recolor's clamp mask differs from the forward's for a non-trivial number of visible Gaussians
        for v in range(V):
            f0, f1 = oracle.forward(scenes[v]), oracle.forward(moved[v])
            n = int(((f0["clamped"] != f1["clamped"]).any(1) & (f0["radii"] > 0)).sum())
            assert n >= 100, (kind, v, n)
            err = np.abs(out[v].cpu().numpy() - f1["out_color"]).max(0)
            assert (err > 1e-4).mean() <= 2e-3, (kind, v)
        args[16] = _t(cp, dev)
        _pin_recolor(N, oracle, moved, args, run, dpix, dev, kind)
        return
    if kind == "colours_shared":
        cols = rng.uniform(-0.2, 1.2, (P, 3)).astype(F)
        per_view = [cols] * V
    else:
        cols = rng.uniform(-0.2, 1.2, (V, P, 3)).astype(F)
        per_view = list(cols)
    _recolor(N, args, run, colours=_t(cols, dev))
    args[2], args[14], args[15] = _t(cols, dev), torch.empty(0), 0
    # per-view colours: dL_dcolor is the sum over the views (gsr.h gsr_forward_recolor)
    _pin_recolor(N, oracle, [with_colours(s, per_view[v], s.bg) for v, s in enumerate(scenes)], args, run, dpix, dev, kind)


def test_colour_backward_after_channels_forward(oracle, gpu_device):
    """gsr_backward_batch after gsr_forward_batch_channels_train: the colour image's gradients alone (gsr.h)"""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    g, views, W, H, scenes = _synth(2, P=12000, W=96, H=80)
    P = scenes[0].P
    args = _args(scenes, dev)
    x = _t(np.random.default_rng(40).normal(0, 1, (P, 8)).astype(F), dev)
    run = N.rasterize_gaussians_batch(*args, need_backward=True, extra=(x, None, _t(np.ones(8, F), dev)))
    assert N.extra_state(run[3]) is not None
    dpix = _dpix(scenes, 41)
    _pin_recolor(N, oracle, scenes, args, run, dpix, dev, "colour backward after a channels forward")


# ------------------------------------------------------------------------------------------------ refused backwards
def test_unsupported_colour_backwards_are_refused(gpu_device):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    g, scenes, args = _recolor_setup(dev)
    V, P, H, W = len(scenes), scenes[0].P, scenes[0].H, scenes[0].W
    dpix = _dpix(scenes, 50)
    run = N.rasterize_gaussians_batch(*args, need_backward=True, capacity=64 * P)
    e = torch.empty(0)

    def bwd(a=args, d=dpix, r=None):
        return _backward(N, a, d, dev, run=run if r is None else r)

    gp0, _, _ = bwd()
    # a forward with need_backward = 0 on the same (full-size) arenas
    _raw_forward(N, args, run, False)
    with pytest.raises(RuntimeError, match=r"last forward on this geometry arena had need_backward = 0"):
        bwd()
    # a need_backward recolor on top of it: no gradient records were cleared, no clamp mask written
    _recolor(N, args, run, campos=args[16])
    with pytest.raises(RuntimeError, match=r"recolor's forward on this geometry arena had need_backward = 0"):
        bwd()
    # a need_backward forward again, then a recolor with need_backward = 0
    _raw_forward(N, args, run, True)
    N.recolor(args[0], args[1], e, args[14], args[15], args[16], H, W, run[0], run[3], run[4], run[5])
    with pytest.raises(RuntimeError, match=r"last gsr_forward_recolor on this geometry arena had need_backward = 0"):
        bwd()
    # back to a need_backward forward: the backward goes through and returns the first call's gradients
    _raw_forward(N, args, run, True)
    gp1, _, _ = bwd()
    util.check_grads(gp1, gp0, "after the refusals", names=("dL_dopacity", "dL_dcolor", "dL_dsh"))
    # V, P, W, H other than the forward's
    one = list(args)
    one[8], one[9], one[16] = args[8][:1], args[9][:1], args[16][:1]
    with pytest.raises(RuntimeError, match=r"V = 1, P = %d, %d x %d, but the last forward or recolor on this geometry arena had "
                                           r"V = 2" % (P, W, H)):
        bwd(one, dpix[:1], run[:2] + (run[2][:1],) + run[3:])
    fewer = list(args)
    fewer[1], fewer[3], fewer[4], fewer[5], fewer[14] = args[1][:-1], args[3][:-1], args[4][:-1], args[5][:-1], args[14][:-1]
    with pytest.raises(RuntimeError, match=r"P = %d, .* had V = 2, P = %d" % (P - 1, P)):
        bwd(fewer, dpix, run[:2] + (run[2][:, :-1].contiguous(),) + run[3:])
    wider = np.zeros((V, 3, H, W + 16), F)
    with pytest.raises(RuntimeError, match=r"P = %d, %d x %d, but" % (P, W + 16, H)):
        bwd(args, wider)
    with pytest.raises(RuntimeError, match=r"P = %d, %d x %d, but" % (P, W, H + 16)):
        bwd(args, np.zeros((V, 3, H + 16, W), F))
    # and the arenas still serve a valid backward
    gp2, _, _ = bwd()
    util.check_grads(gp2, gp0, "after the size refusals", names=("dL_dopacity", "dL_dcolor", "dL_dsh"))
