"""GPU tests (-m gpu) of the opt-in fast arithmetic of the inference forwards (include/gsr.h gsr_set_render_math, csrc/render_math.hpp):

  1. tolerance: on the test scenes the fast mode's images lie within the contract's 1e-4 of the exact mode's except at pixels where an
     alpha or a transmittance threshold falls the other way -- counted, printed and held to the project's share (5e-3) and to four times
     what the reference build's own strict and FMA-contracted variants differ by on the same scene; integer outputs are identical;
  2. the fast mode agrees with itself bit for bit: both forward kernels, a view alone and in a batch, call after call, the extra
     channels against colour forwards of the same values, a colour-only re-render against a full forward;
  3. scope: forwards that save for a backward ignore the switch (bit for bit the exact mode's, and the backward over them passes),
     inference forwards do take it;
  4. the Python surface: render_passes follows set_render_math.

Every test that flips the switch restores it."""
import numpy as np
import pytest
import torch

import util
from native_calls import (RENDER_SCENES as SCENES, RGB_TOL, batch_args as _batch_args, cloud_views as _views_scene, half_views,
                          one_view as _one_view, render_math, renders as _renders, to_device as _t)
from util import build_scene, run_product

pytestmark = pytest.mark.gpu

MAX_FLIP_SHARE = 5e-3     # the project's own bar for threshold flips (test_fma_contraction_moves_few_decisions)
F = np.float32


def _over(a, b):
    """pixels whose largest channel difference exceeds the contract's tolerance, and that difference image"""
    err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max(axis=0)
    return int((err > RGB_TOL).sum()), err


# ---- 1. tolerance against the exact mode -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_fast_mode_is_within_the_contract_of_the_exact_mode(name, gpu_device):
    s, exact, fast = _renders(name, gpu_device)
    strict = util.reference_build("strict").forward(s)
    # the exact mode is still the reference build's, bit for bit (the default has not moved)
    assert exact["out_color"].tobytes() == strict["out_color"].tobytes()
    np.testing.assert_array_equal(exact["radii"], strict["radii"])
    assert exact["R"] == strict["R"]
    # everything in front of the render kernel is untouched by the mode
    np.testing.assert_array_equal(fast["radii"], exact["radii"])
    assert fast["R"] == exact["R"]
    if s.P:
        for k in ("vals", "keys", "ranges", "tiles_touched"):
            assert fast[k].tobytes() == exact[k].tobytes(), k
    # n_ref: what the reference's own two builds (strict order / FMA contraction) differ by on this scene, measured here
    contracted = util.reference_build("fast").forward(s)
    n_ref, err_ref = _over(strict["out_color"], contracted["out_color"])
    n, err = _over(fast["out_color"], exact["out_color"])
    ok = err <= RGB_TOL
    print("%s: fast vs exact: %d of %d pixels over 1e-4 (max %.3g; elsewhere max %.3g, median %.3g); reference strict vs contracted: %d (max %.3g)"
          % (name, n, err.size, err.max(), err[ok].max(initial=0.0), float(np.median(err)), n_ref, err_ref.max()))
    assert np.isfinite(fast["out_color"]).all()
    assert n < MAX_FLIP_SHARE * err.size
    assert n <= max(4, 4 * n_ref)


# ---- 2. the fast mode agrees with itself ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["capsule_circle", "big_splats"])
def test_fast_half_quadrant_kernel_equals_the_fast_8x8_kernel(name, gpu_device):
    s = build_scene(name)
    with render_math(1):
        with half_views(0):
            a, _ = run_product(s, gpu_device, need_backward=False)
        with half_views(1):
            b, _ = run_product(s, gpu_device, need_backward=False)
    for k in ("out_color", "final_T", "n_contrib", "radii"):
        assert a[k].tobytes() == b[k].tobytes(), k
    # (and it is the fast arithmetic both ran: the shared renders are the default single-view path)
    assert b["out_color"].tobytes() == _renders(name, gpu_device)[2]["out_color"].tobytes()


def test_a_view_alone_and_in_a_batch_agree_and_calls_repeat(gpu_device):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    g, views, W, H = _views_scene(3)
    P = g["means3D"].shape[0]
    args = _batch_args(g, views, W, H, dev)
    with render_math(1):
        counts, color, radii, geom, binning, img = N.rasterize_gaussians_batch(*args, need_backward=False)
        state = [[N.query(k, P, W, H, counts[v], geom, binning, img, view=v, n_views=3) for k in ("FINAL_T", "N_CONTRIB")] for v in range(3)]
        for v in range(3):   # (a single view renders on the half-quadrant kernel, the batch on the 8 x 8 one)
            R1, c1, r1, g1, b1, i1 = N.rasterize_gaussians(*_one_view(args, v), need_backward=False)
            assert R1 == counts[v] and torch.equal(r1, radii[v])
            assert torch.equal(c1, color[v]), v
            for k, want in zip(("FINAL_T", "N_CONTRIB"), state[v]):
                assert torch.equal(N.query(k, P, W, H, R1, g1, b1, i1), want), (k, v)
        for _ in range(5):
            again = N.rasterize_gaussians_batch(*args, need_backward=False)
            assert again[0] == counts and torch.equal(again[1], color) and torch.equal(again[2], radii)
    with render_math(0):
        exact = N.rasterize_gaussians_batch(*args, need_backward=False)
    assert not torch.equal(exact[1], color)                    # the fast kernels did run
    assert torch.equal(exact[2], radii) and exact[0] == counts


@pytest.mark.parametrize("nx,layout,scaled", [(nx, layout, scaled) for nx in (4, 8) for layout in ("shared", "per_view", "split")
                                               for scaled in (True, False) if not (nx == 4 and layout == "split")])
def test_fast_extra_channels_equal_fast_colour_forwards(gpu_device, nx, layout, scaled):
    """Each group of three out_extra channels is, bit for bit, the FAST colour forward of colors_precomp = float32(value x scale), and
    out_color the fast colour forward's: one w = alpha T per entry and the same fused multiply-add for every channel, wherever it sits."""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    V = 3
    g, views, W, H = _views_scene(V)
    args = _batch_args(g, views, W, H, dev, bg=(0.25, 0.25, 0.25))
    P = g["means3D"].shape[0]
    rng = np.random.default_rng(31 + nx)
    per_view = _t(rng.normal(0, 1, (V, P, nx)).astype(F), dev)
    if layout == "shared":
        per_view = per_view[:1].expand(V, P, nx).contiguous()
        values = per_view[0].contiguous()
    elif layout == "per_view":
        values = per_view
    else:
        per_view[:, :, :4] = per_view[0, :, :4].clone()
        values = (per_view[0, :, :4].contiguous(), per_view[:, :, 4:].contiguous())
    scale = _t(rng.choice([-1.0, 1.0, 0.5], (V, nx)).astype(F), dev) if scaled else None
    bgx = _t(rng.uniform(0, 1, nx).astype(F), dev)
    e = torch.empty(0)
    with render_math(1):
        counts, color, radii, geom, binning, img, out_x = N.rasterize_gaussians_batch(*args, need_backward=False, extra=(values, scale, bgx))
        c0, color0, radii0 = N.rasterize_gaussians_batch(*args, need_backward=False)[:3]
        assert counts == c0 and torch.equal(radii, radii0)
        assert torch.equal(color, color0)
        for k0 in range(0, nx, 3):
            ks = [min(k0 + i, nx - 1) for i in range(3)]
            for v in range(V):
                cols = per_view[v][:, ks]
                if scaled:
                    cols = cols * scale[v, ks]
                a = _one_view(args, v)
                a[0] = bgx[ks].contiguous()
                a[2], a[14] = cols.contiguous(), e                           # colors_precomp instead of SHs
                ref = N.rasterize_gaussians(*a, need_backward=False)[1]
                assert torch.equal(out_x[v, ks], ref), (k0, v)
    with render_math(0):
        assert not torch.equal(N.rasterize_gaussians_batch(*args, need_backward=False, extra=(values, scale, bgx))[6], out_x)


@pytest.mark.parametrize("name", ["capsule_circle", "culled_mix"])
def test_fast_recolor_equals_a_full_fast_forward(name, gpu_device):
    from diff_gaussian_rasterization import _native as N
    from oracle.oracle import Scene
    dev = gpu_device
    s = build_scene(name)
    e = torch.empty(0)
    args = (_t(s.bg, dev), _t(s.means3D, dev), e, _t(s.opacities, dev), _t(s.scales, dev), _t(s.rotations, dev), 1.0, e,
            _t(s.viewmatrix.reshape(4, 4), dev), _t(s.projmatrix.reshape(4, 4), dev), s.tanfovx, s.tanfovy, s.H, s.W,
            _t(s.shs, dev), s.sh_degree, _t(s.campos, dev), False, False)
    colors = np.random.default_rng(5).uniform(-1, 1, s.means3D.shape).astype(F)
    s2 = Scene(W=s.W, H=s.H, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=s.bg, means3D=s.means3D, opacities=s.opacities,
               viewmatrix=s.viewmatrix, projmatrix=s.projmatrix, campos=s.campos, colors_precomp=colors, scales=s.scales,
               rotations=s.rotations)
    with render_math(1):
        R, rgb, radii, geom, binning, img = N.rasterize_gaussians(*args, need_backward=False)
        got = N.recolor(args[0], args[1], _t(colors, dev), e, 0, args[16], s.H, s.W, R, geom, binning, img).cpu().numpy()
        want = run_product(s2, dev, need_backward=False)[0]["out_color"]
        again = N.recolor(args[0], args[1], e, args[14], s.sh_degree, args[16], s.H, s.W, R, geom, binning, img)
    assert got.tobytes() == want.tobytes()
    assert torch.equal(again, rgb)
    with render_math(0):
        exact = run_product(s2, dev, need_backward=False)[0]["out_color"]
    assert got.tobytes() != exact.tobytes()


# ---- 3. scope ------------------------------------------------------------------------------------------------------------------
def test_training_forwards_ignore_the_switch(gpu_device):
    """need_backward = True: the exact kernels whatever the switch says -- image, final_T and n_contrib bit for bit the exact mode's,
    and the backward over that forward passes against the reference build."""
    s = build_scene("capsule_circle")
    dL = util.seeded_dL(s)
    with render_math(0):
        a, _ = run_product(s, gpu_device, dL_dpix=dL)
    with render_math(1):
        b, gb = run_product(s, gpu_device, dL_dpix=dL)
    for k in ("out_color", "final_T", "n_contrib", "radii"):
        assert a[k].tobytes() == b[k].tobytes(), k
    _, gr = util.reference_build("strict").forward_backward(s, dL)
    gr = dict(gr)
    gr["dL_dopacity"] = gr["dL_dopacity"].reshape(gb["dL_dopacity"].shape)
    util.check_grads(gb, gr, "capsule_circle, backward over a forward with the fast switch on (ref)")


@pytest.mark.parametrize("nx", [4, 8])
def test_channels_train_forward_ignores_the_switch(gpu_device, nx):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    V = 2
    g, views, W, H = _views_scene(V)
    args = _batch_args(g, views, W, H, dev, bg=(0.25, 0.25, 0.25))
    P = g["means3D"].shape[0]
    rng = np.random.default_rng(7)
    x = _t(rng.normal(0, 1, (P, nx)).astype(F), dev)
    scale = _t(rng.choice([-1.0, 1.0, 0.5], (V, nx)).astype(F), dev)
    bgx = _t(rng.uniform(0, 1, nx).astype(F), dev)

    def run():
        r = N.rasterize_gaussians_batch(*args, need_backward=True, extra=(x, scale, bgx))
        st = [N.query(k, P, W, H, r[0][v], r[3], r[4], r[5], view=v, n_views=V) for k in ("FINAL_T", "N_CONTRIB") for v in range(V)]
        return r, st
    with render_math(0):
        a, sa = run()
    with render_math(1):
        b, sb = run()
        inference = N.rasterize_gaussians_batch(*args, need_backward=False, extra=(x, scale, bgx))
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[6], b[6])
    for p, q in zip(sa, sb):
        assert torch.equal(p, q)
    assert not torch.equal(inference[6], a[6]) and not torch.equal(inference[1], a[1])   # (the same call without need_backward does switch)


def test_inference_forward_takes_the_switch(gpu_device):
    """capsule_circle with the switch on differs from the exact image in at least one bit: the fast kernel really ran."""
    s, exact, fast = _renders("capsule_circle", gpu_device)
    assert exact["out_color"].tobytes() != fast["out_color"].tobytes()
    assert exact["final_T"].tobytes() != fast["final_T"].tobytes() or (exact["out_color"] != fast["out_color"]).any()


def test_debug_mode_runs_clean_in_fast_mode(gpu_device):
    s, _, fast = _renders("capsule_circle", gpu_device)
    with render_math(1):
        d, _ = run_product(s, gpu_device, debug=True, need_backward=False)
    assert d["out_color"].tobytes() == fast["out_color"].tobytes()


# ---- 4. Python -----------------------------------------------------------------------------------------------------------------
def test_render_passes_follows_set_render_math(gpu_device):
    import diff_gaussian_rasterization as d
    from pcrender import raster_passes as rp, camera, synth
    dev = gpu_device
    cloud = synth.make_cloud("synth-THuman-256", seed=0, P=20000)
    g = synth.make_gaussians(cloud, profile="inference", seed=1)
    sf = cloud["scale_factor"]
    radius = np.sqrt(3) / sf * 6
    means, shs = _t(g["means3D"], dev), _t(g["shs"], dev)
    opac, rots = _t(g["opacities"], dev), _t(g["rotations"], dev)
    decoded_s = _t((g["scales"] / radius).astype(F), dev)
    normals = torch.nn.functional.normalize(means, dim=-1)
    Hs = camera.circle_path(12, 0, 3, [90, 0])
    h = w = 128
    bg = torch.ones(3)

    def passes():
        return rp.render_passes(means, opac, decoded_s, rots, shs, Hs, h, w, 45.0, bg, sf, normals=normals, sh_degree=1, super_sample_rate=2)
    was = d.get_render_math()
    try:
        assert d.set_render_math("exact") == "exact" and d.get_render_math() == "exact"
        exact = passes()
        assert d.set_render_math("fast") == "fast" and d.get_render_math() == "fast"
        fast = passes()
        fast2 = passes()
    finally:
        d.set_render_math(was)
    assert d.get_render_math() == was
    differs = False
    for k in ("rgb", "xyz_w", "hitmap", "normal"):
        assert fast[k].shape == (1, 12, h, w, 3) == exact[k].shape
        assert torch.equal(fast[k], fast2[k]), k
        err = (fast[k].double() - exact[k].double()).abs().amax(dim=-1)     # largest channel difference per (view, pixel)
        n = int((err > RGB_TOL).sum())
        print("render_passes %s: %d of %d pixels over 1e-4 after the down-filter (max %.3g)" % (k, n, err.numel(), float(err.max())))
        assert n < MAX_FLIP_SHARE * err.numel(), k
        differs = differs or not torch.equal(fast[k], exact[k])
    assert differs
