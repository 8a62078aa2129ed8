"""The deterministic channels backward (gsr_backward_batch_channels_det; diff_gaussian_rasterization.set_deterministic_channels):
every output -- the eight per-Gaussian gradients, the per-view records and dL_dextra_values -- bit-identical from call to call and
from process to process, the same values as the atomic channels backward up to the order of float additions (held to the float64
reference at the bars the atomic path is held to), the C ABI's contract, and the Python switch.

Run as a script (`python tests/test_gpu_deterministic_channels.py --child OUT_DIR`) this file is the child process of the
repeatability test: it renders every case afresh and writes its deterministic results to OUT_DIR/<case>.npz."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "gaussian-pcloud-render_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, _p)

import util  # noqa: E402
from fp64_channels import channels_backward_fp64_scenes, fold_extra  # noqa: E402
from fp64_pins import (channel_inputs as _inputs, deep_stack_cloud as _deep_stack, flat64 as _flat, flipped_view as _flip,  # noqa: E402
                       rel_err as _err, synth_scenes as _synth, view_settings as _settings)
from native_calls import (channels_backward_args, circle_scene as _scene, longest_list as _long_lists, moments,  # noqa: E402
                          scene_args as _args, to_device as _t)
from sweep_support import power_scene, same_bits as _same  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = util.GRAD_NAMES
EXTRA = "dL_dextra_values"


def _dev_inputs(x, sc, bgx, dev):
    xt = tuple(_t(a, dev) for a in x) if isinstance(x, tuple) else _t(x, dev)
    return xt, None if sc is None else _t(sc, dev), _t(bgx, dev)


def _forward(N, args, xt, sct, bgxt, capacity=None):
    """channels forward with need_backward: (counts, color, radii, geom, binning, img, out_x)"""
    return N.rasterize_gaussians_batch(*args, need_backward=True, extra=(xt, sct, bgxt), capacity=capacity)


def _backward(N, args, run, xt, sct, bgxt, dpix, dx, det, dev, **kw):
    """one channels backward on the arenas of `run`: the eight per-Gaussian gradients, the per-view records and dL_dextra_values
    (flat, in the layout of the values) as numpy arrays: ten tensors"""
    counts, color, radii, geom, binning, img = run[:6]
    g = N.rasterize_gaussians_backward_channels_batch(*channels_backward_args(args, run, _t(dpix, dev), (xt, sct, bgxt), _t(dx, dev), 1.0),
                                                      deterministic=det, **kw)
    out = {n: t.detach().cpu().numpy() for n, t in zip(NAMES, g[:8])}
    gx = g[8]
    out[EXTRA] = (torch.cat([gx[0].reshape(-1), gx[1].reshape(-1)]) if isinstance(gx, tuple) else gx.reshape(-1)).cpu().numpy()
    P, V = args[1].shape[0], dpix.shape[0]
    out["records"] = np.stack([N.grad_records(geom, P, view=v, n_views=V).cpu().numpy() for v in range(V)])
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> builder() -> dict(scenes, x, dense, sc, bgx, dpix, dx, layout, mode, check): host data only, so that parent and child build
# the same case and the float64 reference can be taken from it; check(N, run) asserts what the case is there for
def _pack(scenes, nx, layout, seed, mode=None, check=None, no_scale=False):
    s = scenes[0]
    x, dense, sc, bgx, dpix, dx = _inputs(s.P, len(scenes), nx, layout, seed=seed, H=s.H, W=s.W)
    return dict(scenes=scenes, x=x, dense=dense, sc=None if no_scale else sc, bgx=bgx, dpix=dpix, dx=dx, layout=layout, mode=mode,
                check=check)


def _case_layout(layout, nx):
    def build():
        scenes = _synth(2, P=12000, W=96, H=80)[4]
        c = _pack(scenes, nx, layout, seed=300 + 10 * layout + nx)
        assert (c["sc"] == 0).any() and (c["sc"] < 0).any()             # the drawn view scales include 0 and negatives
        return c
    return build


def _case_modes(mode):
    def build():
        g, views, W, H = _scene(3, P=12000, W=208, H=176)
        return _pack([util.scene_from(g, v, W, H, bg=(0.1, 0.2, 0.3)) for v in views], 8, 2, seed=5, mode=mode)
    return build


def _case_deep(V, P):
    def build():
        g, W, H = _deep_stack(P, 13)
        cam = util.identity_camera(W, H)
        scenes = [util.scene_from(g, cam, W, H, bg=(0.2, 0.3, 0.4)) for _ in range(V)]

        def check(N, run):   # the list reaches the capped last slice (512-entry slices at V = 1, 1024 from V = 2 on)
            counts, _, _, geom, binning, img = run[:6]
            assert _long_lists(N, geom, binning, img, counts, P, W, H, V) > 32 << (9 if V == 1 else 10)
        return _pack(scenes, 4, 1, seed=40 + V, check=check)
    return build


def _case_empty_middle():
    g, views, W, H = _scene(3, P=12000, W=96, H=80)
    views = [views[0], _flip(views[1]), views[2]]

    def check(N, run):
        assert run[0][1] == 0 and run[0][0] > 0 and run[0][2] > 0
    return _pack([util.scene_from(g, v, W, H, bg=(0.1, 0.2, 0.3)) for v in views], 8, 1, seed=52, check=check)


def _case_no_scale():
    return _pack(_synth(2, P=12000, W=96, H=80)[4], 4, 0, seed=31, no_scale=True)


def _case_precomp():
    g, views, W, H = _scene(2, P=8000, W=96, H=80)
    g = dict(g)
    g["colors_precomp"] = np.random.default_rng(4).uniform(0, 1, (g["means3D"].shape[0], 3)).astype(F)
    return _pack([util.scene_from(g, v, W, H, bg=(0.5, 0.2, 0.1), mode="colors", use_cov3d=True) for v in views], 8, 2, seed=14)


PULLED = (12, 20000, 1024, 704)


def _case_pulled():
    V, P, W, H = PULLED
    g, views, W, H = _scene(V, P=P, W=W, H=H)
    return _pack([util.scene_from(g, v, W, H, bg=(0.0, 0.0, 0.0)) for v in views], 8, 2, seed=77)


FP64_CASES = ("layout_0_nx8", "layout_1_nx8", "layout_2_nx8", "capped_last_slice_v1", "capped_last_slice_v2")
CASES = {"layout_%d_nx%d" % (lay, nx): _case_layout(lay, nx) for lay, nx in ((0, 8), (1, 8), (2, 8), (0, 4), (1, 4))}
CASES.update({
    "moments_mode_0": _case_modes(0), "moments_mode_1": _case_modes(1), "moments_mode_2": _case_modes(2),
    "capped_last_slice_v1": _case_deep(1, 20000), "capped_last_slice_v2": _case_deep(2, 36000),
    "empty_middle_view": _case_empty_middle, "no_view_scale": _case_no_scale, "precomputed_cov_and_colours": _case_precomp,
    "pulled_work_units": _case_pulled,
})


def _run_case(N, dev, name, repeats, atomic=0):
    """one forward, `repeats` deterministic backwards over it (then `atomic` atomic ones): (case, deterministic results, atomic)"""
    with moments(None):
        c = CASES[name]()
        if c["mode"] is not None:
            assert N.lib.gsr_set_backward_moments(c["mode"]) == c["mode"]
        args = _args(c["scenes"], dev)
        xt, sct, bgxt = _dev_inputs(c["x"], c["sc"], c["bgx"], dev)
        run = _forward(N, args, xt, sct, bgxt)
        if c["check"] is not None:
            c["check"](N, run)
        bw = lambda det: _backward(N, args, run, xt, sct, bgxt, c["dpix"], c["dx"], det, dev)  # noqa: E731
        return c, [bw(True) for _ in range(repeats)], [bw(False) for _ in range(atomic)]


@pytest.fixture(scope="module")
def child_results(tmp_path_factory):
    """every case rendered afresh and differentiated once in ONE child process (a fresh HIP context, its own allocations)"""
    out = str(tmp_path_factory.mktemp("det_channels_child"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out


def test_the_pulled_units_case_takes_the_pulled_units():
    """render_bwd.hip launch_render_backward: batches whose static grid would exceed GSR_BWD_FILL = 4096 groups pull their units"""
    V, P, W, H = PULLED
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    assert V > 1 and tiles % 8 == 0 and (tiles // 8) * V == 4224 > 4096
    assert ((208 + 15) // 16) * ((176 + 15) // 16) // 8 * 3 <= 4096      # the moments-mode cases take the static quartets


@pytest.mark.parametrize("name", sorted(CASES))
def test_repeatable_from_call_to_call_and_from_process_to_process(gpu_device, child_results, name):
    from diff_gaussian_rasterization import _native as N
    c, runs, _ = _run_case(N, gpu_device, name, 5)
    assert len(runs[0]) == 10
    for i, r in enumerate(runs[1:]):
        bad = [k for k in r if not np.array_equal(runs[0][k].view(np.uint32), r[k].view(np.uint32))]
        assert not bad, "%s: deterministic channels backward %d differs from the first in %s" % (name, i + 2, bad)
    with np.load(os.path.join(child_results, name + ".npz")) as z:
        child = {k: z[k] for k in z.files}
    assert sorted(child) == sorted(runs[0])
    bad = [k for k in child if not np.array_equal(runs[0][k].view(np.uint32), child[k].view(np.uint32))]
    assert not bad, "%s: a fresh forward + backward in another process gave other bits in %s" % (name, bad)
    assert all(np.isfinite(v).all() for v in runs[0].values())
    assert runs[0][EXTRA].any() and runs[0]["records"].any()
    if name == "empty_middle_view":
        V, P = 3, c["scenes"][0].P
        gx = runs[0][EXTRA].reshape(V, P, 8)
        assert not gx[1].any() and gx[0].any() and gx[2].any()           # the empty view's rows of a per-view output: exactly zero
        assert not runs[0]["records"][1].any()


# ---------------------------------------------------------------------------------------------------------------- same values
@pytest.mark.parametrize("name", FP64_CASES)
def test_same_values_as_the_atomic_path_against_float64(oracle, gpu_device, name):
    """the deterministic call passes the comparison the atomic call passes in tests/test_gpu_channels_fp64.py (_compare_batch):
    util.check_grads' bars on opacity / colour / dL_dextra / dL_dopacity / dL_dcolor, 1e-5 of max|g| on mean2D / conic -- and the
    deterministic results against the atomic ones of the same forward at util.check_grads' bars"""
    from diff_gaussian_rasterization import _native as N
    c, det, atomic = _run_case(N, gpu_device, name, 1, atomic=1)
    det, atomic = det[0], atomic[0]
    want = channels_backward_fp64_scenes(oracle, c["scenes"], c["dense"], c["sc"], c["bgx"], c["dpix"], c["dx"])
    for v in range(len(c["scenes"])):
        w, r = want["views"][v], det["records"][v].astype(np.float64)
        util.check_grads({"opacity": r[:, 8:9], "colour": r[:, 5:8]}, {"opacity": w["opacity"][:, None], "colour": w["colour"]},
                         "%s view %d" % (name, v), names=("opacity", "colour"))
        e2, ec = _err(r[:, 0:2], w["mean2D"]), _err(r[:, 2:5], w["conic"])
        print("%s view %d: mean2D %.3e, conic %.3e of max|g| against float64" % (name, v, e2, ec))
        assert e2 <= 1e-5 and ec <= 1e-5, (name, v, e2, ec)
    gxo = _flat(fold_extra(np.stack([w["extra"] for w in want["views"]]), c["layout"]))
    util.check_grads({"dL_dextra": det[EXTRA].astype(np.float64).reshape(-1, 1)}, {"dL_dextra": gxo.reshape(-1, 1)}, name,
                     names=("dL_dextra",))
    util.check_grads({"dL_dopacity": det["dL_dopacity"], "dL_dcolor": det["dL_dcolor"]},
                     {"dL_dopacity": want["grads"]["dL_dopacity"], "dL_dcolor": want["grads"]["dL_dcolor"]}, name,
                     names=("dL_dopacity", "dL_dcolor"))
    both = NAMES + (EXTRA,)
    util.check_grads({k: det[k].reshape(-1, 1) if k == EXTRA else det[k] for k in both},
                     {k: atomic[k].reshape(-1, 1) if k == EXTRA else atomic[k] for k in both}, name + ", deterministic vs atomic",
                     names=both)


# ------------------------------------------------------------------------------------------------------- does the scene tell?
def test_power_scene_with_eight_extra_channels(gpu_device):
    """Five atomic channels backwards on the colour test's power scene: how many elements of dL_dextra_values differ between pairs
    is printed, not asserted (profiles/r13_det_channels_backward.txt records it); five deterministic ones are identical."""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    s = power_scene()
    x, dense, sc, bgx, dpix, dx = _inputs(s.P, 1, 8, 0, seed=8, H=s.H, W=s.W)
    args = _args([s], dev)
    xt, sct, bgxt = _dev_inputs(x, sc, bgx, dev)
    run = _forward(N, args, xt, sct, bgxt)
    atomic = [_backward(N, args, run, xt, sct, bgxt, dpix, dx, False, dev) for _ in range(5)]
    differing = [int((a[EXTRA].view(np.uint32) != b[EXTRA].view(np.uint32)).sum()) for i, a in enumerate(atomic) for b in atomic[i + 1:]]
    other = [sum(int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum()) for k in NAMES) for i, a in enumerate(atomic) for b in atomic[i + 1:]]
    print("power scene, eight extra channels: elements of dL_dextra_values (of %d) that differ between pairs of atomic channels "
          "backwards: %s; of the eight gradients: %s" % (atomic[0][EXTRA].size, differing, other))
    det = [_backward(N, args, run, xt, sct, bgxt, dpix, dx, True, dev) for _ in range(5)]
    assert all(_same(det[0], d) for d in det[1:])
    both = NAMES + (EXTRA,)
    util.check_grads({k: det[0][k].reshape(-1, 1) if k == EXTRA else det[0][k] for k in both},
                     {k: atomic[0][k].reshape(-1, 1) if k == EXTRA else atomic[0][k] for k in both},
                     "power scene, deterministic vs atomic", names=both)


# ------------------------------------------------------------------------------------------------------------------ contract
def test_contract_of_the_c_abi(gpu_device, monkeypatch):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    N.selftest(dev)                                                      # (includes the extras' reduction against host sums)
    scenes = _synth(2, P=8000, W=96, H=80)[4]
    s = scenes[0]
    P, V, W, H = s.P, 2, s.W, s.H
    x, dense, sc, bgx, dpix, dx = _inputs(P, V, 8, 2, seed=60, H=H, W=W)
    dx2 = np.random.default_rng(61).uniform(-1, 1, dx.shape).astype(F)
    args = _args(scenes, dev)
    xt, sct, bgxt = _dev_inputs(x, sc, bgx, dev)
    run = _forward(N, args, xt, sct, bgxt, capacity=64 * P)
    pairs = N.last_list_pairs(V)
    need = int(N.lib.gsr_backward_det_channels_bytes(V, P, W, H, pairs, 8, 2))
    bw = lambda d, **kw: _backward(N, args, run, xt, sct, bgxt, dpix, d, True, dev, **kw)  # noqa: E731
    # no device->host read-back in a deterministic channels backward
    torch.cuda.synchronize()
    before = N.lib.gsr_d2h_count()
    a1 = bw(dx)
    torch.cuda.synchronize()
    assert N.lib.gsr_d2h_count() == before
    # every call returns the gradients of ITS dL_dextra, whatever ran before it on the arenas
    b2, a3, b4 = bw(dx2), bw(dx), bw(dx2)
    assert _same(a1, a3) and _same(b2, b4)
    assert not np.array_equal(a1[EXTRA], b2[EXTRA]) and not np.array_equal(a1["dL_dmean2D"], b2["dL_dmean2D"])
    atomic2 = _backward(N, args, run, xt, sct, bgxt, dpix, dx2, False, dev)
    both = NAMES + (EXTRA,)
    util.check_grads({k: b2[k].reshape(-1, 1) if k == EXTRA else b2[k] for k in both},
                     {k: atomic2[k].reshape(-1, 1) if k == EXTRA else atomic2[k] for k in both}, "second dL_dextra", names=both)
    # a block of exactly the stated size, sized by the lists' exact extent and full of NaN bytes: nothing of it reaches an output
    real = N.det_scratch
    monkeypatch.setattr(N, "det_scratch", lambda *a: torch.full((need,), 0xFF, dtype=torch.uint8, device=dev))
    assert _same(a1, bw(dx))
    # one byte short: refused with the needed size in the message, outputs untouched
    made = []

    def alloc(shape, dtype=None, device=None):
        made.append(torch.full(shape, -7.5, dtype=dtype, device=device))
        return made[-1]
    monkeypatch.setattr(N, "det_scratch", lambda *a: torch.empty((need - 1,), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match=r"scratch block too small \(%d < %d = gsr_backward_det_channels_bytes\(2, %d, %d, %d, %d, 8, 2\)"
                       % (need - 1, need, P, W, H, pairs)):
        bw(dx, _alloc=alloc)
    torch.cuda.synchronize()
    assert len(made) == 9 and all(bool((t == -7.5).all()) for t in made)
    # a block sized for the colour entry only is too small as well
    small = int(N.lib.gsr_backward_det_bytes(V, P, W, H, pairs))
    assert small < need
    monkeypatch.setattr(N, "det_scratch", lambda *a: torch.empty((small,), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match=r"scratch block too small \(%d < %d" % (small, need)):
        bw(dx)
    monkeypatch.setattr(N, "det_scratch", real)
    # and the arenas still serve a deterministic backward with the first one's bits
    assert _same(a1, bw(dx))


# -------------------------------------------------------------------------------------------------------------------- Python
@pytest.fixture
def channels_on():
    import diff_gaussian_rasterization as d
    was, was_x = d.get_deterministic(), d.get_deterministic_channels()
    d.set_deterministic_channels(True)
    yield d
    d.set_deterministic(was)
    d.set_deterministic_channels(was_x)


def test_python_rasterize_views_channels(gpu_device, channels_on):
    d, dev = channels_on, gpu_device
    from diff_gaussian_rasterization import _native as N
    V = 2
    g, views, W, H = _scene(V, P=8000, W=96, H=80)
    P = g["means3D"].shape[0]
    sts = _settings(views, W, H, (0.0, 0.0, 0.0), dev, g["sh_degree"])
    rng = np.random.default_rng(80)
    lo, hi = rng.normal(0, 1, (P, 4)).astype(F), rng.normal(0, 1, (V, P, 4)).astype(F)
    bgx, sc = _t(rng.uniform(-1, 1, 8).astype(F), dev), _t(rng.choice([-2.0, 0.0, 0.5, 3.0], (V, 8)).astype(F), dev)
    dpix, dx = _t(rng.uniform(-1, 1, (V, 3, H, W)).astype(F), dev), _t(rng.uniform(-1, 1, (V, 8, H, W)).astype(F), dev)
    names = ("means3D", "means2D", "shs", "opacities", "scales", "rotations", "lo", "hi")

    def once():
        L = {k: _t(g[k], dev).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        L["means2D"] = torch.zeros((P, 3), device=dev, requires_grad=True)
        L["lo"], L["hi"] = _t(lo, dev).requires_grad_(True), _t(hi, dev).requires_grad_(True)
        color, _, ex = d.rasterize_views_channels(L["means3D"], L["means2D"], L["opacities"], sts, (L["lo"], L["hi"]), bgx,
                                                  extra_view_scale=sc, shs=L["shs"], scales=L["scales"], rotations=L["rotations"])
        ((color * dpix).sum() + (ex * dx).sum()).backward()
        return color.detach(), ex.detach(), {k: L[k].grad.detach().clone() for k in names}

    for forced in (None, True):          # fully deterministic whatever set_deterministic says
        d.set_deterministic(forced)
        out = []
        for _ in range(3):
            before = dict(N.CALLS)
            out.append(once())
            assert N.CALLS["backward_channels_det"] == before["backward_channels_det"] + 1
            assert N.CALLS["backward"] == before["backward"] and N.CALLS["backward_det"] == before["backward_det"]
        for o in out[1:]:
            assert all(torch.equal(out[0][2][k], o[2][k]) for k in names)
    d.set_deterministic(None)
    d.set_deterministic_channels(False)  # the switch off: the atomic entry, the same forward images, gradients at the usual bars
    before = dict(N.CALLS)
    color, ex, grads = once()
    assert N.CALLS["backward_channels_det"] == before["backward_channels_det"]
    assert torch.equal(color, out[0][0]) and torch.equal(ex, out[0][1])
    flat = lambda t: t.cpu().numpy().reshape(-1, 1) if t.dim() != 2 else t.cpu().numpy()  # noqa: E731
    checked = ("shs", "opacities", "lo", "hi")
    util.check_grads({k: flat(out[0][2][k]) for k in checked}, {k: flat(grads[k]) for k in checked}, "switch on vs off", names=checked)


def test_python_train_passes(gpu_device, channels_on):
    d, dev = channels_on, gpu_device
    from diff_gaussian_rasterization import _native as N
    from pcrender import camera, raster_passes as rp, synth
    cloud = synth.make_cloud("synth-THuman-256", seed=0, P=4000)
    g = synth.make_gaussians(cloud, profile="inference", seed=1)
    sf = cloud["scale_factor"]
    radius = np.sqrt(3) / sf * 6
    Hs = camera.circle_path(2, 0, 3, [90, 0])
    h = w = 64
    bg = torch.zeros(3, device=dev)
    rng = np.random.default_rng(81)
    weights = dict(xyz_w=1.0, rgb=0.01, hitmap=0.01, normal=10.0)
    R = {k: _t(rng.uniform(-1, 1, (1, 2, h, w, 3)).astype(F), dev) for k in weights}
    names = ("means3D", "opacities", "scales", "rotations", "shs", "normals")

    def once():
        leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
        L = dict(means3D=leaf(g["means3D"]), opacities=leaf(g["opacities"]), scales=leaf((g["scales"] / radius).astype(F)),
                 rotations=leaf(g["rotations"]), shs=leaf(g["shs"]))
        L["normals"] = torch.nn.functional.normalize(_t(g["means3D"], dev) + 0.1, dim=-1).requires_grad_(True)
        out = rp.train_passes(L["means3D"], L["opacities"], L["scales"], L["rotations"], L["shs"], Hs, h, w, 45.0, bg, sf,
                              normals=L["normals"], sh_degree=1, super_sample_rate=1)
        sum(weights[k] * (out[k] * R[k]).sum() for k in weights).backward()
        return {k: v.detach() for k, v in out.items()}, {k: L[k].grad.detach().clone() for k in names}

    out = []
    for _ in range(3):
        before = N.CALLS["backward_channels_det"]
        out.append(once())
        assert N.CALLS["backward_channels_det"] == before + 1
    for o in out[1:]:
        assert all(torch.equal(out[0][1][k], o[1][k]) for k in names)
    assert all(bool(torch.isfinite(v).all()) and bool(v.any()) for v in out[0][1].values())
    d.set_deterministic_channels(False)
    before = N.CALLS["backward_channels_det"]
    images, _ = once()
    assert N.CALLS["backward_channels_det"] == before
    assert all(torch.equal(images[k], out[0][0][k]) for k in images)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    from diff_gaussian_rasterization import _native as _N
    _dev = torch.device("cuda:0")
    for _name in sorted(CASES):
        np.savez(os.path.join(sys.argv[2], _name + ".npz"), **_run_case(_N, _dev, _name, 1)[1][0])
    torch.cuda.synchronize()
