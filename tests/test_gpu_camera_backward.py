"""gsr_backward_cameras (csrc/camera_bwd.hip) on the GPU: dL/d viewmatrix, projmatrix and campos after each kind of backward, held to
the float64 arbiter of tests/fp64_camera.py (bar: camera_cases.hold), to the translation identity on the library's own outputs, to
bit equality where the contract promises it, and through the Python layers (rasterize_views_cameras, rasterize_views_posed).
Outputs are prefilled with NaN and the scratch block with 0xFF bytes before every call: an output that is not written, or a slab
word that is read without having been written, shows."""
import numpy as np
import pytest
import torch

import camera_cases as CC
import util
from camera_sweep import _bits, _cameras, _prefilled
from native_calls import channels_backward_args, colour_backward_args, follower_args, scene_args as _args, to_device as _t

pytestmark = pytest.mark.gpu

F = np.float32
TALLY = dict(exits=0, live=0, worst=0.0)      # over the cases held to the arbiter in this file


def _forward(N, args, need_backward=True):
    counts, color, radii, geom, binning, img = N.rasterize_gaussians_batch(*args, need_backward=need_backward)
    return radii, geom, binning, img


def _backward(N, args, run, dpix, deterministic=False):
    return N.rasterize_gaussians_backward_batch(*colour_backward_args(args, (None, None) + tuple(run), dpix), deterministic=deterministic)


def _hold(cams, ref, tag):
    worst = 0.0
    for v, c in enumerate(cams):
        exits, w = CC.hold(c, ref["exact"][v], ref["yard"][v], "%s view %d" % (tag, v))
        TALLY["exits"] += exits
        TALLY["live"] += CC.N_LIVE
        worst = max(worst, w)
    TALLY["worst"] = max(TALLY["worst"], worst)
    print("%s: worst |lib - exact| / plain bar = %.4g" % (tag, worst))


def _run_case(N, name, dev, deterministic=False):
    ref = CC.reference(name)
    args = _args(ref["scenes"], dev)
    run = _forward(N, args)
    g = _backward(N, args, run, _t(np.stack(ref["dLs"]), dev), deterministic=deterministic)
    return ref, args, run, g


@pytest.mark.parametrize("name", CC.ARBITER_CASES)
def test_against_the_arbiter(gpu_device, name):
    """one Gaussian (255 idle lanes); block edges (V = 3, SH degree 2); the mixed cloud (a view that sees nothing, Gaussians behind the
    camera, outside the frustum clamp, clamped SH channels; degrees 0 and 3; cov3D_precomp + colors_precomp)"""
    from diff_gaussian_rasterization import _native as N
    ref, args, run, _ = _run_case(N, name, gpu_device)
    cams = _cameras(N, args, run[0], run[1])
    _hold(cams, ref, name)
    if name.startswith("mixed"):
        for n, _, _ in CC.TENSORS:
            assert (cams[1][n].view(np.uint32) == 0).all(), "%s: the view that sees nothing must get +0 everywhere (%s)" % (name, n)
    if name in ("mixed_sh0", "mixed_precomp"):
        for c in cams:
            assert (c["dL_dcampos"].view(np.uint32) == 0).all(), name


def _identity(scenes, g, cams, P, tag):
    """the translation identity on the library's own outputs.  Both sides are float32 results of P-term signed sums (the left one's
    terms were rounded to float32 one by one, the right one's sums once), so they agree to P * 2^-24 * sum_i |dL_dmean3D[i][j]|."""
    gm = g[3].cpu().numpy().astype(np.float64)
    left, right = CC.translation_identity(scenes, gm, cams)
    bound = P * 2.0 ** -24 * np.abs(gm).sum(0)
    print("%s: translation identity |left - right| = %s, bound %s, |left| = %s" % (tag, np.abs(left - right), bound, np.abs(left)))
    assert (np.abs(gm).sum(0) > 0).all()
    assert (np.abs(left - right) <= bound).all(), (tag, left, right, bound)


def test_many_partials(gpu_device):
    """more partials than k_camera_sum has threads, with a ragged end: held to the translation identity and to bit equality"""
    from diff_gaussian_rasterization import _native as N
    P, W, H = CC.MANY_PARTIALS_P, 64, 64
    rng = np.random.default_rng(5)
    g = CC.cloud(P, 51, 1, xy=0.55, scale=(0.003, 0.006))        # tiny splats ...
    g["scales"][:400] = rng.uniform(0.1, 0.3, (400, 3))          # ... and a few of ordinary size
    g["opacities"][:] = rng.uniform(0.02, 0.08, (P, 1))
    scenes = CC.views_of(g, [CC.pose(3)], W, H)
    args = _args(scenes, gpu_device)
    run = _forward(N, args)
    grads = _backward(N, args, run, _t(util.seeded_dL(scenes[0])[None], gpu_device))
    assert int((run[0] > 0).sum()) > P // 2
    a = _cameras(N, args, run[0], run[1])
    b = _cameras(N, args, run[0], run[1])
    assert _bits(a) == _bits(b), "two calls over one backward differ"
    for n, live, dead in CC.TENSORS:
        assert (a[0][n][dead].view(np.uint32) == 0).all() and np.abs(a[0][n][live]).max() > 0, n
    _identity(scenes, grads, a, P, "many partials")


def test_translation_identity_over_three_views(gpu_device):
    from diff_gaussian_rasterization import _native as N
    name = "edges_%d" % CC.EDGE_SIZES[-1]
    ref, args, run, g = _run_case(N, name, gpu_device)
    _identity(ref["scenes"], g, _cameras(N, args, run[0], run[1]), ref["scenes"][0].P, name)


def test_after_a_channels_backward(gpu_device):
    """nx = 4, V = 2: the records carry the extras' share, and so does the camera gradient"""
    from diff_gaussian_rasterization import _native as N
    ref = CC.reference("channels")
    scenes, dev = ref["scenes"], gpu_device
    args = _args(scenes, dev)
    x, sc, bgx, dx = CC.channels_inputs(scenes)
    extra = (_t(x, dev), _t(sc, dev), _t(bgx, dev))
    dpix = _t(np.stack(ref["dLs"]), dev)
    counts, color, radii, geom, binning, img, out_x = N.rasterize_gaussians_batch(*args, need_backward=True, extra=extra)
    run = (counts, color, radii, geom, binning, img)
    N.rasterize_gaussians_backward_channels_batch(*channels_backward_args(args, run, dpix, extra, _t(dx, dev), 1.0))
    cams = _cameras(N, args, radii, geom)
    _hold(cams, ref, "channels")
    run = _forward(N, args)
    _backward(N, args, run, dpix)
    colour_only = _cameras(N, args, run[0], run[1])
    for v in range(len(scenes)):
        for n in ("dL_dviewmatrix", "dL_dprojmatrix"):
            d = np.abs(cams[v][n].astype(np.float64) - colour_only[v][n]).max()
            assert d > 100 * util.GRAD_ABS * np.abs(ref["exact"][v][n]).max(), "the extras' share did not arrive (view %d %s)" % (v, n)


def test_deterministic(gpu_device):
    """after gsr_backward_batch_det: bit-identical camera gradients from round to round, and from call to call over one backward"""
    from diff_gaussian_rasterization import _native as N
    name = "edges_%d" % CC.EDGE_SIZES[-1]
    rounds = []
    for _ in range(2):
        ref, args, run, _g = _run_case(N, name, gpu_device, deterministic=True)
        first = _cameras(N, args, run[0], run[1])
        again = _cameras(N, args, run[0], run[1])
        assert _bits(first) == _bits(again)
        rounds.append(first)
    assert _bits(rounds[0]) == _bits(rounds[1])
    _hold(rounds[0], ref, name + " (deterministic)")


def test_second_backward(gpu_device):
    """backward with dL_dpix A, cameras, backward with B, cameras: the second result is B's (the records are cleared in between)"""
    from diff_gaussian_rasterization import _native as N
    name = "edges_%d" % CC.EDGE_SIZES[2]
    ref = CC.reference(name)
    args = _args(ref["scenes"], gpu_device)
    run = _forward(N, args)
    A = np.random.default_rng(3).uniform(-1, 1, np.stack(ref["dLs"]).shape).astype(F)
    _backward(N, args, run, _t(A, gpu_device))
    first = _cameras(N, args, run[0], run[1])
    _backward(N, args, run, _t(np.stack(ref["dLs"]), gpu_device))
    second = _cameras(N, args, run[0], run[1])
    assert _bits(first) != _bits(second)
    _hold(second, ref, name + " (second backward)")


def test_refusals_that_need_a_record(gpu_device):
    from diff_gaussian_rasterization import _native as N
    ref = CC.reference("edges_%d" % CC.EDGE_SIZES[0])
    dev = gpu_device
    args = _args(ref["scenes"], dev)
    P, V = ref["scenes"][0].P, len(ref["scenes"])

    def refused(radii, geom, message, views=V):
        out, scratch = _prefilled(N, views, P, dev)
        with pytest.raises(RuntimeError, match=message):
            N.backward_cameras(*follower_args(args, radii, geom, views), _out=out, _scratch=scratch)
        torch.cuda.synchronize()
        for o in out:
            assert torch.isnan(o).all(), "a refused call wrote an output"

    run = _forward(N, args)
    refused(run[0], run[1], "no backward has run since the last forward or recolor")
    _backward(N, args, run, _t(np.stack(ref["dLs"]), dev))
    refused(run[0], run[1], r"V = 2, P = %d, 70 x 50, but the last forward or recolor .* had V = 3" % P, views=2)
    _cameras(N, args, run[0], run[1])                     # (the matching call goes through)
    run0 = _forward(N, args, need_backward=False)
    refused(run0[0], run0[1], "had need_backward = 0")
    run = _forward(N, args)                               # a new forward on arenas of its own: its record starts without a backward
    refused(run[0], run[1], "no backward has run since")


def test_exits_stay_rare():
    """over the whole file at most 1 in 20 live entries may need the 4 x yardstick exit (tests/test_cpu_camera_cases.py shows that the
    yardstick itself needs none)"""
    print("camera gradients: %d of %d live entries needed the 4 x yardstick exit; worst |lib - exact| / plain bar = %.4g"
          % (TALLY["exits"], TALLY["live"], TALLY["worst"]))
    assert TALLY["exits"] * 20 <= TALLY["live"], TALLY


# ---- the Python layers ----------------------------------------------------------------------------------------------------
def _settings(scenes, dev):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return [GaussianRasterizationSettings(
        image_height=s.H, image_width=s.W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=_t(s.bg, dev), scale_modifier=1.0,
        viewmatrix=_t(s.viewmatrix.reshape(4, 4), dev), projmatrix=_t(s.projmatrix.reshape(4, 4), dev), sh_degree=s.sh_degree,
        campos=_t(s.campos, dev), prefiltered=False, debug=False) for s in scenes]


def test_rasterize_views_cameras(gpu_device):
    """images and cloud gradients are rasterize_views' bit for bit; the cameras' .grad is the direct C-ABI result (all under the
    deterministic backward, so that two backwards of one forward give the same bits)"""
    import diff_gaussian_rasterization as d
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    ref = CC.reference("edges_%d" % CC.EDGE_SIZES[2])
    scenes, s = ref["scenes"], ref["scenes"][0]
    sts = _settings(scenes, dev)
    dL = _t(np.stack(ref["dLs"]), dev)
    old = N.get_deterministic()
    N.set_deterministic(True)
    try:
        def leaves():
            out = [_t(a, dev).requires_grad_(True) for a in (s.means3D, s.opacities.reshape(-1, 1), s.shs, s.scales, s.rotations)]
            return out + [torch.zeros_like(out[0], requires_grad=True)]

        m, o, sh, sc, ro, m2 = leaves()
        img_a, radii_a = d.rasterize_views(m, m2, o, sts, shs=sh, scales=sc, rotations=ro)
        (img_a * dL).sum().backward()
        want = [t.grad.clone() for t in (m, o, sh, sc, ro, m2)]

        view, proj, cam = (torch.stack([getattr(st, n).reshape(shape) for st in sts]).clone().requires_grad_(True)
                           for n, shape in (("viewmatrix", (4, 4)), ("projmatrix", (4, 4)), ("campos", (3,))))
        m, o, sh, sc, ro, m2 = leaves()
        before = N.CALLS["backward_cameras"]
        img_b, radii_b = d.rasterize_views_cameras(m, m2, o, sts, view, proj, cam, shs=sh, scales=sc, rotations=ro)
        (img_b * dL).sum().backward()
        assert N.CALLS["backward_cameras"] == before + 1
        assert torch.equal(img_a, img_b) and torch.equal(radii_a, radii_b)
        for w, t in zip(want, (m, o, sh, sc, ro, m2)):
            assert w.cpu().numpy().tobytes() == t.grad.cpu().numpy().tobytes()
        assert view.grad.shape == (3, 4, 4) and proj.grad.shape == (3, 4, 4) and cam.grad.shape == (3, 3)

        args = _args(scenes, dev)
        run = _forward(N, args)
        _backward(N, args, run, dL, deterministic=True)
        direct = _cameras(N, args, run[0], run[1])
        got = [dict(dL_dviewmatrix=view.grad[v].reshape(16).cpu().numpy(), dL_dprojmatrix=proj.grad[v].reshape(16).cpu().numpy(),
                    dL_dcampos=cam.grad[v].cpu().numpy()) for v in range(3)]
        assert _bits(got) == _bits(direct)

        # no camera input needs a gradient: the extra call is not made
        m, o, sh, sc, ro, m2 = leaves()
        before = N.CALLS["backward_cameras"]
        img_c, _ = d.rasterize_views_cameras(m, m2, o, sts, view.detach(), proj.detach(), cam.detach(), shs=sh, scales=sc, rotations=ro)
        (img_c * dL).sum().backward()
        assert N.CALLS["backward_cameras"] == before and torch.equal(img_c, img_a)
    finally:
        N.set_deterministic(old)


def test_rasterize_views_posed(gpu_device):
    """H_c2w.grad of an ordinary loss.backward() against the arbiter's 35 values per view pulled back through
    raster_settings_tensors by float64 autograd on the host; the bar of camera_cases.hold on the 12 live entries of each pose"""
    from grad_ladder import Float64
    from pcrender import camera, raster_passes
    dev = gpu_device
    q, w, h, fov = 2, 70, 50, 60.0
    g = CC.cloud(500, 41, 2, scale=(0.1, 0.3))
    H32 = torch.stack([CC.pose(3), CC.pose(8)])
    H = H32.to(dev).requires_grad_(True)
    leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
    m = leaf(g["means3D"])
    imgs = raster_passes.rasterize_views_posed(m, leaf(g["opacities"]), leaf(g["scales"]), leaf(g["rotations"]), H, h, w, fov,
                                               shs=leaf(g["shs"]), sh_degree=2, super_sample_rate=1)
    assert tuple(imgs.shape) == (1, q, h, w, 3)
    dLs = [np.random.default_rng(60 + v).uniform(-1, 1, (3, h, w)).astype(F) for v in range(q)]
    (imgs * _t(np.stack(dLs), dev).permute(0, 2, 3, 1)[None]).sum().backward()
    lib = H.grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(lib).all() and m.grad is not None

    # the scenes the rasterizer saw: the matrices as the device computed them
    with torch.no_grad():
        a = camera.raster_settings_tensors(H32.to(dev), w, h, fov, 1)
    views = [dict(tanfovx=a["tanfovx"], tanfovy=a["tanfovy"], viewmatrix=a["viewmatrix"][v].cpu().numpy(),
                  projmatrix=a["projmatrix"][v].cpu().numpy(), campos=a["campos"][v].cpu().numpy()) for v in range(q)]
    scenes = [util.scene_from(g, vw, w, h) for vw in views]
    f64 = Float64(scenes, dLs)

    def pulled_back(sums, dtype):
        cg = [CC.camera_backward_fp64(s_, w_["fwd"]["radii"], w_["fwd"]["clamped"], w_[sums]["dL_dmean2D"], w_[sums]["dL_dconic"],
                                      w_[sums]["dL_dcolor"], dtype=dtype) for s_, w_ in zip(scenes, f64.views())]
        Hd = H32.double().requires_grad_(True)
        r = camera.raster_settings_tensors(Hd, w, h, fov, 1)
        tot = sum((r[k].reshape(q, -1) * torch.from_numpy(np.stack([np.asarray(c[n], np.float64).reshape(-1) for c in cg]))).sum()
                  for k, n in (("viewmatrix", "dL_dviewmatrix"), ("projmatrix", "dL_dprojmatrix"), ("campos", "dL_dcampos")))
        tot.backward()
        return Hd.grad.numpy()

    exact, yard = pulled_back("exact", np.float64), pulled_back("grads32", np.float32)
    exits = 0
    for v in range(q):
        assert (lib[v, 3] == 0).all()
        x, y, e = exact[v, :3], np.abs(yard[v, :3] - exact[v, :3]), np.abs(lib[v, :3] - exact[v, :3])
        plain = util.GRAD_ABS * np.abs(x).max()
        print("posed view %d: worst |lib - exact| / plain bar = %.4g" % (v, e.max() / plain))
        assert (e <= np.maximum(plain, 4 * y)).all(), (v, e.max(), plain, (4 * y).max())
        exits += int((e > plain).sum())
    assert exits * 20 <= 12 * q
