"""The deterministic colour backward (gsr_backward_batch_det; diff_gaussian_rasterization.set_deterministic): bit-identical
gradients from call to call and from process to process, the same values as the atomic backward up to the order of float additions,
the C ABI's contract, and the Python switch.

Run as a script (`python tests/test_gpu_deterministic_backward.py --child OUT_DIR`) this file is the child process of the
repeatability test: it renders every case afresh and writes its deterministic gradients to OUT_DIR/<case>.npz."""
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
from fp64_pins import (colour_fp64 as _fp64, deep_stack_cloud as _deep_stack, flipped_view as _flip,  # noqa: E402
                       raw_forward as _raw_forward, rel_err as _err, synth_scenes as _synth, view_settings as _settings)
from native_calls import (circle_scene as _scene, cloud_args as _cloud_args, longest_list as _long_lists, moments,  # noqa: E402
                          scene_args as _args, to_device as _t)
from sweep_support import (leaves as _leaves, nine_tensors_backward as _backward, power_scene, same_bits as _same,  # noqa: E402
                           uniform_dpix as _dpix)

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = util.GRAD_NAMES
GOLDEN = sorted(f[4:-4] for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.startswith("ref_") and f.endswith(".npz"))


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> builder(N, dev) -> (args, run, dpix, moments mode or None); parent and child build them the same way
def _case_golden(name):
    def build(N, dev):
        s = util.build_scene(name)
        args = _args([s], dev)
        return args, N.rasterize_gaussians_batch(*args, need_backward=True), _dpix(1, s.H, s.W, 3), None
    return build


def _case_views(V, P, W, H, mode=None, seed=4):
    def build(N, dev):
        g, views, W_, H_ = _scene(V, P=P, W=W, H=H)
        args = _cloud_args(g, views, W, H, dev, (0.1, 0.2, 0.3))
        return args, N.rasterize_gaussians_batch(*args, need_backward=True), _dpix(V, H, W, seed), mode
    return build


def _case_deep(V, P):
    def build(N, dev):
        g, W, H = _deep_stack(P, 17)
        cam = util.identity_camera(W, H)
        scenes = [util.scene_from(g, cam, W, H, bg=(0.2, 0.3, 0.4)) for _ in range(V)]
        args = _args(scenes, dev)
        run = N.rasterize_gaussians_batch(*args, need_backward=True)
        counts, _, _, geom, binning, img = run
        # the list reaches the capped last slice (512-entry slices at V = 1, 1024 from V = 2 on)
        assert _long_lists(N, geom, binning, img, counts, P, W, H, V) > 32 << (9 if V == 1 else 10)
        return args, run, _dpix(V, H, W, 60 + V), None
    return build


def _case_empty_middle(N, dev):
    g, views, W, H = _scene(3, P=12000, W=96, H=80)
    views = [views[0], _flip(views[1]), views[2]]
    scenes = [util.scene_from(g, v, W, H, bg=(0.1, 0.2, 0.3)) for v in views]
    args = _args(scenes, dev)
    run = N.rasterize_gaussians_batch(*args, need_backward=True)
    assert run[0][1] == 0 and run[0][0] > 0 and run[0][2] > 0
    return args, run, _dpix(3, H, W, 12), None


def _case_precomp(N, dev):
    g, views, W, H = _scene(2, P=8000, W=96, H=80)
    g = dict(g)
    g["colors_precomp"] = np.random.default_rng(4).uniform(0, 1, (g["means3D"].shape[0], 3)).astype(F)
    scenes = [util.scene_from(g, v, W, H, bg=(0.5, 0.2, 0.1), mode="colors", use_cov3d=True) for v in views]
    args = _args(scenes, dev)
    return args, N.rasterize_gaussians_batch(*args, need_backward=True), _dpix(2, H, W, 14), None


def _case_recolor(N, dev):
    g, views, W, H = _scene(2, P=8000, W=96, H=80)
    scenes = [util.scene_from(g, v, W, H, bg=(0.2, 0.2, 0.6)) for v in views]
    args = list(_args(scenes, dev))
    run = N.rasterize_gaussians_batch(*args, need_backward=True)
    cols = _t(np.random.default_rng(30).uniform(-0.2, 1.2, (scenes[0].P, 3)).astype(F), dev)
    e = torch.empty(0)
    N.recolor(args[0], args[1], cols, e, 0, args[16], H, W, run[0], run[3], run[4], run[5], need_backward=True)
    args[2], args[14], args[15] = cols, e, 0
    return args, run, _dpix(2, H, W, 31), None


def _case_channels_train(N, dev):
    g, views, W, H, scenes = _synth(2, P=12000, W=96, H=80)
    args = _args(scenes, dev)
    x = _t(np.random.default_rng(40).normal(0, 1, (scenes[0].P, 8)).astype(F), dev)
    run = N.rasterize_gaussians_batch(*args, need_backward=True, extra=(x, None, _t(np.ones(8, F), dev)))
    assert N.extra_state(run[3]) is not None
    return args, run, _dpix(2, H, W, 41), None


FULL = (12, 200_000, 1920, 1080)
CASES = {"golden_" + n: _case_golden(n) for n in GOLDEN}
CASES.update({
    "one_view_static": _case_views(1, 40000, 320, 240),
    "three_views": _case_views(3, 12000, 208, 176),
    "twelve_views_1080p": _case_views(*FULL),
    "capped_last_slice_v1": _case_deep(1, 20000), "capped_last_slice_v2": _case_deep(2, 36000),
    "empty_middle_view": _case_empty_middle, "precomputed_cov_and_colours": _case_precomp,
    "moments_mode_0": _case_views(3, 12000, 208, 176, mode=0, seed=5), "moments_mode_1": _case_views(3, 12000, 208, 176, mode=1, seed=5),
    "moments_mode_2": _case_views(3, 12000, 208, 176, mode=2, seed=5),
    "after_recolor": _case_recolor, "after_channels_train": _case_channels_train,
})


def _run_case(N, dev, name, repeats):
    """one forward, `repeats` deterministic backwards over it"""
    with moments(None):
        args, run, dpix, mode = CASES[name](N, dev)
        if mode is not None:
            assert N.lib.gsr_set_backward_moments(mode) == mode
        return [_backward(N, args, run, dpix, True, dev) for _ in range(repeats)]


@pytest.fixture(scope="module")
def child_results(tmp_path_factory):
    """every case rendered afresh and differentiated once in ONE child process (a fresh HIP context, its own allocations)"""
    out = str(tmp_path_factory.mktemp("det_child"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out


def test_the_full_size_case_takes_the_pulled_units():
    """render_bwd.hip launch_render_backward: batches whose static grid would exceed 4096 groups of workgroups pull their units"""
    V, P, W, H = FULL
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    assert V > 1 and ((tiles + 7) // 8) * V > 4096
    assert ((208 + 15) // 16) * ((176 + 15) // 16) // 8 * 3 <= 4096      # "three_views" takes the static quartets, as every V = 1 call


@pytest.mark.parametrize("name", sorted(CASES))
def test_repeatable_from_call_to_call_and_from_process_to_process(gpu_device, child_results, name):
    from diff_gaussian_rasterization import _native as N
    runs = _run_case(N, gpu_device, name, 5)
    assert len(runs[0]) == 9
    for i, r in enumerate(runs[1:]):
        assert _same(runs[0], r), "%s: deterministic backward %d differs from the first" % (name, i + 2)
    with np.load(os.path.join(child_results, name + ".npz")) as z:
        child = {k: z[k] for k in z.files}
    assert sorted(child) == sorted(runs[0])
    assert _same(runs[0], child), "%s: a fresh forward + backward in another process gave other bits" % name
    assert all(np.isfinite(v).all() for v in runs[0].values())


# ------------------------------------------------------------------------------------------------------- the scene can tell
def test_the_atomic_path_is_visibly_not_repeatable_on_the_power_scene(gpu_device):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    s = power_scene()
    args = _args([s], dev)
    run = N.rasterize_gaussians_batch(*args, need_backward=True)
    dpix = _dpix(1, s.H, s.W, 2)
    atomic = [_backward(N, args, run, dpix, False, dev) for _ in range(5)]
    differing = [sum(int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum()) for k in NAMES)
                 for i, a in enumerate(atomic) for b in atomic[i + 1:]]
    print("power scene: elements that differ between pairs of atomic backwards:", differing)
    assert any(d > 0 for d in differing), "scene has no power"
    det = [_backward(N, args, run, dpix, True, dev) for _ in range(5)]
    assert all(_same(det[0], d) for d in det[1:])
    util.check_grads(det[0], {k: atomic[0][k] for k in NAMES}, "power scene, deterministic vs atomic", names=NAMES)


# ---------------------------------------------------------------------------------------------------------------- same values
@pytest.mark.parametrize("name", GOLDEN)
def test_edge_scenes_pass_the_existing_bars(oracle, gpu_device, name):
    """the deterministic gradients against the oracle and against the reference build, at the bars of tests/util.py"""
    import diff_gaussian_rasterization as d
    s = util.build_scene(name)
    dL = util.seeded_dL(s)
    was = d.get_deterministic()
    try:
        d.set_deterministic(True)
        from diff_gaussian_rasterization import _native as N
        before = N.CALLS["backward_det"]
        _, gp = util.run_product(s, gpu_device, dL)
        assert N.CALLS["backward_det"] == before + 1
    finally:
        d.set_deterministic(was)
    _, go = oracle.forward_backward(s, dL)
    util.check_grads(gp, go, name + " (oracle)")
    _, gr = util.reference_build().forward_backward(s, dL)
    util.check_grads(gp, gr, name + " (reference build)")


def test_one_full_size_view_passes_the_existing_bars(gpu_device):
    """one 1920 x 1080 view of the 200 K cloud: deterministic against the reference build's backward"""
    import diff_gaussian_rasterization as d
    g, views, W, H = _scene(1, P=200_000, W=1920, H=1080)
    s = util.scene_from(g, views[0], W, H, bg=(0.0, 0.0, 0.0))
    dL = util.seeded_dL(s)
    was = d.get_deterministic()
    try:
        d.set_deterministic(True)
        _, gp = util.run_product(s, gpu_device, dL, light=True)
    finally:
        d.set_deterministic(was)
    _, gr = util.reference_build().forward_backward(s, dL)
    util.check_grads(gp, gr, "full-size view (reference build)")


FP64_SCENES = ["random_aniso", "culled_mix", "opaque_early_stop", "deep_stack", "big_splats"]
METRICS = ("mean2D", "conic", "colour", "opacity")


def test_error_against_float64_is_the_atomic_path_s(oracle, gpu_device):
    """Against the float64 render backward (the oracle's, per view) the deterministic records are held to the atomic records of the
    same build on the same scenes.  The yardstick is the atomic path (median over the scenes of the max-element error, per run);
    the margin is the spread its five runs show: det <= max(atomic) + (max(atomic) - min(atomic)), per moments mode and quantity.
    Observed ratios deterministic / median atomic: profiles/r08_deterministic_backward.txt.

    MISSED on the MI355X by one of the twelve figures in two of four sessions (it held in the other two); the bar stays as set.
      session 1: mode 2 conic,  deterministic 4.9717e-07, atomic 4.9709e-07 in all five runs (1.00016x)
      session 2: mode 1 colour, deterministic 2.2889e-07, atomic 2.2638e-07 in all five runs (1.011x)
      (the other figures: ratios 0.87 .. 1.35 of the median atomic run, each inside max + spread)
    Why (per scene, ten atomic runs each, profiles/r08_deterministic_backward.txt): the max-element error of a scene is set by ONE
    element, and on most of these scenes that element's atomic sum is the same in every run -- one partial sum, or a few whose
    waves of one quartet arrive in the same order every time -- so the atomic figure takes one value (or two to eight) and its
    five-run spread, the margin, is often exactly zero.  On such an element the reduction's float64 sum, rounded once, is the
    correctly rounded sum of the same float32 partials and differs from the float32 running sum in the last bit: closer to float64
    on some (random_aniso mode 0 conic 1.14e-07 against 1.33e-07; opaque_early_stop mode 2 colour 2.17e-07 against 2.74e-07),
    farther on others (random_aniso mode 0 colour 1.57e-07 against 1.36e-07; opaque_early_stop mode 1 opacity 2.51e-07 against
    2.07e-07), each time against an atomic figure without spread.  Which of the twelve medians lands on such a pair decides the
    session.  The partial sums are shared and the final rounding is the best float32 allows: there is nothing left in the
    reduction to make more exact."""
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    g, views, W, H, batch = _synth(3, P=12000, W=96, H=80)
    cases = [(n, [util.build_scene(n)]) for n in FP64_SCENES] + [("synth V=3", batch)]
    sl = dict(mean2D=slice(0, 2), conic=slice(2, 5), colour=slice(5, 8), opacity=slice(8, 9))
    errs = {m: {k: {"det": [], "atomic": [[] for _ in range(5)]} for k in METRICS} for m in (0, 1, 2)}
    with moments(None):
        for name, scenes in cases:
            dpix = _dpix(len(scenes), scenes[0].H, scenes[0].W, 7 + len(name))
            want = _fp64(oracle, scenes, dpix)["views"]
            args = _args(scenes, dev)
            run = N.rasterize_gaussians_batch(*args, need_backward=True)

            def err(rec, k):
                w = [x[k][:, None] if x[k].ndim == 1 else x[k] for x in want]
                return max(_err(rec[v][:, sl[k]].astype(np.float64), w[v]) for v in range(len(scenes)))
            for m in (0, 1, 2):
                assert N.lib.gsr_set_backward_moments(m) == m
                rec = _backward(N, args, run, dpix, True, dev)["records"]
                for k in METRICS:
                    errs[m][k]["det"].append(err(rec, k))
                for r in range(5):
                    rec = _backward(N, args, run, dpix, False, dev)["records"]
                    for k in METRICS:
                        errs[m][k]["atomic"][r].append(err(rec, k))
    bad = []
    for m in (0, 1, 2):
        for k in METRICS:
            det = float(np.median(errs[m][k]["det"]))
            at = [float(np.median(a)) for a in errs[m][k]["atomic"]]
            print("moments mode %d, %-7s: deterministic %.3e, atomic runs %.3e .. %.3e (median %.3e): ratio %.3f" % (
                m, k, det, min(at), max(at), float(np.median(at)), det / max(float(np.median(at)), 1e-30)))
            if not det <= max(at) + (max(at) - min(at)):
                bad.append((m, k, det, min(at), max(at)))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ contract
def test_contract_of_the_c_abi(gpu_device, monkeypatch):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    g, views, W, H = _scene(2, P=8000, W=96, H=80)
    scenes = [util.scene_from(g, v, W, H, bg=(0.2, 0.2, 0.6)) for v in views]
    args = _args(scenes, dev)
    P, V = scenes[0].P, 2
    dpix = _dpix(V, H, W, 50)
    N.selftest(dev)
    run = N.rasterize_gaussians_batch(*args, need_backward=True, capacity=64 * P)
    pairs = N.last_list_pairs(V)
    need = int(N.lib.gsr_backward_det_bytes(V, P, W, H, pairs))
    # no device->host read-back in a deterministic backward
    torch.cuda.synchronize()
    before = N.lib.gsr_d2h_count()
    good = _backward(N, args, run, dpix, True, dev)
    torch.cuda.synchronize()
    assert N.lib.gsr_d2h_count() == before
    # a block of exactly the stated size is accepted; one byte short is refused with the needed size in the message
    real = N.det_scratch
    monkeypatch.setattr(N, "det_scratch", lambda *a: torch.empty((need,), dtype=torch.uint8, device=dev))
    assert _same(good, _backward(N, args, run, dpix, True, dev))
    monkeypatch.setattr(N, "det_scratch", lambda *a: torch.empty((need - 1,), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match=r"scratch block too small \(%d < %d" % (need - 1, need)):
        _backward(N, args, run, dpix, True, dev)
    monkeypatch.setattr(N, "det_scratch", real)
    # gsr_backward_batch's refusals hold for the new entry
    _raw_forward(N, args, run, False)
    with pytest.raises(RuntimeError, match=r"last forward on this geometry arena had need_backward = 0"):
        _backward(N, args, run, dpix, True, dev)
    _raw_forward(N, args, run, True)
    one = list(args)
    one[8], one[9], one[16] = args[8][:1], args[9][:1], args[16][:1]
    with pytest.raises(RuntimeError, match=r"V = 1, P = %d, %d x %d, but the last forward or recolor on this geometry arena had V = 2" % (P, W, H)):
        _backward(N, one, run[:2] + (run[2][:1],) + run[3:], dpix[:1], True, dev)
    with pytest.raises(RuntimeError, match=r"P = %d, %d x %d, but" % (P, W + 16, H)):
        _backward(N, args, run, np.zeros((V, 3, H, W + 16), F), True, dev)
    # and the arenas still serve a deterministic backward with the first one's bits
    assert _same(good, _backward(N, args, run, dpix, True, dev))


# -------------------------------------------------------------------------------------------------------------------- Python
LEAVES = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")


def _grads(L):
    return {k: L[k].grad.detach().clone() for k in LEAVES}


@pytest.fixture
def forced_on():
    import diff_gaussian_rasterization as d
    was = d.get_deterministic()
    d.set_deterministic(True)
    yield d
    d.set_deterministic(was)


def test_python_rasterize_views_twelve_views(gpu_device, forced_on):
    d, dev = forced_on, gpu_device
    from diff_gaussian_rasterization import _native as N
    g, views, W, H = _scene(12, P=12000, W=208, H=176)
    sts = _settings(views, W, H, (0.1, 0.1, 0.1), dev, g["sh_degree"])
    dpix = _t(_dpix(12, H, W, 70), dev)
    out = []
    for _ in range(2):
        L = _leaves(g, dev)
        before = dict(N.CALLS)
        color, _ = d.rasterize_views(L["means3D"], L["means2D"], L["opacities"], sts, shs=L["shs"], scales=L["scales"],
                                     rotations=L["rotations"])
        (color * dpix).sum().backward()
        assert N.CALLS["backward_det"] == before["backward_det"] + 1 and N.CALLS["backward"] == before["backward"]
        out.append(_grads(L))
    assert all(torch.equal(out[0][k], out[1][k]) for k in LEAVES)
    # retain_graph: two backwards over one forward
    L = _leaves(g, dev)
    color, _ = d.rasterize_views(L["means3D"], L["means2D"], L["opacities"], sts, shs=L["shs"], scales=L["scales"], rotations=L["rotations"])
    loss = (color * dpix).sum()
    loss.backward(retain_graph=True)
    first = _grads(L)
    for k in LEAVES:
        L[k].grad = None
    loss.backward()
    assert all(torch.equal(first[k], L[k].grad) for k in LEAVES) and all(torch.equal(first[k], out[0][k]) for k in LEAVES)
    # the switch off: the old entry
    d.set_deterministic(False)
    L = _leaves(g, dev)
    before = dict(N.CALLS)
    color, _ = d.rasterize_views(L["means3D"], L["means2D"], L["opacities"], sts, shs=L["shs"], scales=L["scales"], rotations=L["rotations"])
    (color * dpix).sum().backward()
    assert N.CALLS["backward"] == before["backward"] + 1 and N.CALLS["backward_det"] == before["backward_det"]


def test_python_per_view_rasterizer(gpu_device, forced_on):
    """GaussianRasterizer per view (the general path on the first frame of a configuration, then the short path)"""
    d, dev = forced_on, gpu_device
    from diff_gaussian_rasterization import _native as N
    g, views, W, H = _scene(1, P=12000, W=208, H=176)
    st = _settings(views, W, H, (0.1, 0.1, 0.1), dev, g["sh_degree"])[0]
    dpix = _t(_dpix(1, H, W, 71)[0], dev)
    out = []
    for _ in range(4):
        L = _leaves(g, dev)
        before = dict(N.CALLS)
        color, _ = d.GaussianRasterizer(st)(means3D=L["means3D"], means2D=L["means2D"], shs=L["shs"], opacities=L["opacities"],
                                            scales=L["scales"], rotations=L["rotations"])
        loss = (color * dpix).sum()
        loss.backward(retain_graph=True)
        first = _grads(L)
        for k in LEAVES:
            L[k].grad = None
        loss.backward()
        assert all(torch.equal(first[k], L[k].grad) for k in LEAVES)
        assert N.CALLS["backward_det"] == before["backward_det"] + 2 and N.CALLS["backward"] == before["backward"]
        out.append(first)
    for o in out[1:]:
        assert all(torch.equal(out[0][k], o[k]) for k in LEAVES)


def test_python_channels_call_raises_when_forced_on(gpu_device, forced_on):
    d, dev = forced_on, gpu_device
    g, views, W, H = _scene(2, P=2000, W=96, H=80)
    sts = _settings(views, W, H, (0.0, 0.0, 0.0), dev, g["sh_degree"])
    L = _leaves(g, dev)
    x = torch.zeros((2000, 4), device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="no deterministic backward"):
        d.rasterize_views_channels(L["means3D"], L["means2D"], L["opacities"], sts, x, torch.zeros(4, device=dev), shs=L["shs"],
                                   scales=L["scales"], rotations=L["rotations"])


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    from diff_gaussian_rasterization import _native as _N
    _dev = torch.device("cuda:0")
    for _name in sorted(CASES):
        np.savez(os.path.join(sys.argv[2], _name + ".npz"), **_run_case(_N, _dev, _name, 1)[0])
    torch.cuda.synchronize()
