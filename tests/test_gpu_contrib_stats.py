"""gsr_contrib_stats (csrc/contrib_stats.hip) on the GPU, held to the host reference of tests/contrib_ref.py: the counts inside their
brackets (equal where the bracket is closed: every case here has at most 2 % open ones, tests/test_cpu_contrib_ref.py), weight_max
inside [max_lo (1 - e), max_hi (1 + e)], weight_sum within the float32 summation bar of the oracle's float64 sum, the total against
the oracle's sum of 1 - final_T.  Every output is prefilled before every call (NaN, or a sentinel for the integers): a row that is not
written, or not cleared, shows.  The cases are the smallest at which the kernel can go wrong: one Gaussian, partial tiles, a Gaussian
over six tiles, lists longer than a staging round, a stop after two entries, invisible Gaussians, three views, weight maps."""
import numpy as np
import pytest
import torch

import contrib_ref as R
from native_calls import colour_backward_args, contrib_stats_args, scene_args as _args, scene_settings as _settings, to_device as _t

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -12345
NAMES = R.NAMES
EXACT = ("weight_max", "pixel_count", "dominant_count")     # the bit-reproducible outputs


def _forward(N, args, need_backward=False):
    return N.rasterize_gaussians_batch(*args, need_backward=need_backward)


def _prefilled(P, dev, old=None):
    if old is None:
        return [torch.full((P,), float("nan"), device=dev), torch.full((P,), float("nan"), device=dev),
                torch.full((P,), SENTINEL, dtype=torch.int32, device=dev), torch.full((P,), SENTINEL, dtype=torch.int32, device=dev)]
    return [_t(np.asarray(old[n]), dev) for n in NAMES]


def _contrib(N, args, run, weights=None, old=None, want=NAMES, V=None, out=None, radii=True):
    """one gsr_contrib_stats call for the outputs named in `want` (the others NULL): dict of numpy arrays"""
    dev = args[1].device
    V = args[8].shape[0] if V is None else V
    out = _prefilled(args[1].shape[0], dev, old) if out is None else out
    o = {n: (t if n in want else None) for n, t in zip(NAMES, out)}
    N.contrib_stats(*contrib_stats_args(args, run, V, radii), accumulate=old is not None,
                    pixel_weights=None if weights is None else _t(weights, dev), **o)
    return {n: t.cpu().numpy() for n, t in o.items() if t is not None}


def _bits(d, names=EXACT):
    return b"".join(np.ascontiguousarray(d[n]).tobytes() for n in names)


def _case(N, name, dev, need_backward=False, **kw):
    c = R.case(name, **kw)
    args = _args(c["scenes"], dev)
    run = _forward(N, args, need_backward)
    return c, args, run


def test_one_gaussian_against_the_hand_values(gpu_device):
    from diff_gaussian_rasterization import _native as N
    c, args, run = _case(N, "one", gpu_device)
    got = _contrib(N, args, run)
    (s, mx, n, dom), = R.hand_values(c["ref"]["fwd"][0], 16, 16)
    assert got["pixel_count"].tolist() == [n] and got["dominant_count"].tolist() == [dom] and n == dom == 16
    assert abs(float(got["weight_max"][0]) - mx) <= 5 * 2.0 ** -24 * mx
    assert abs(float(got["weight_sum"][0]) - s) <= (n + 6) * 2.0 ** -24 * s
    R.check(got, c["ref"], "one")
    R.check_total(got["weight_sum"], c["ref"], "one")


@pytest.mark.parametrize("name", ["two", "partial_17x16", "partial_40x24", "stack300", "opaque70", "behind"])
def test_edge_shapes(gpu_device, name):
    """partial tiles and the inside mask; one Gaussian over six tiles (atomics across tiles and quadrants); lists longer than a staging
    round; a stop after two entries; Gaussians behind the camera and off screen"""
    from diff_gaussian_rasterization import _native as N
    c, args, run = _case(N, name, gpu_device)
    ref = c["ref"]
    got = _contrib(N, args, run)
    R.check(got, ref, name)
    R.check_total(got["weight_sum"], ref, name)
    radii = run[2].cpu().numpy()
    assert np.array_equal(radii[0] > 0, ref["visible"])
    for n in NAMES:                                   # consistent with radii == 0: exact zeros
        assert not got[n][radii[0] <= 0].view(np.uint32).any(), n
    if name == "partial_40x24":
        assert got["pixel_count"][0] == 40 * 24
    if name == "stack300":
        assert (got["pixel_count"] > 0).all()
    if name == "opaque70":
        assert (got["pixel_count"][:2] == 256).all() and got["dominant_count"][0] == 256
        for n in NAMES:
            assert not got[n][2:].view(np.uint32).any(), "an entry behind the stop got something in " + n
    if name == "behind":
        assert (radii[0] <= 0).sum() >= 10
    # a NULL radii changes nothing, and every subset of the outputs gives the same bits
    again = _contrib(N, args, run, radii=False)
    assert _bits(again) == _bits(got)
    for want in (("weight_sum",), ("weight_max",), ("pixel_count",), ("dominant_count",), ("weight_max", "dominant_count")):
        part = _contrib(N, args, run, want=want)
        assert tuple(part) == want
        for n in want:
            if n in EXACT:
                assert part[n].tobytes() == got[n].tobytes(), (want, n)
        R.check(part, ref, "%s %s" % (name, want))


def test_three_views_are_the_sum_of_three_calls_and_accumulate_adds(gpu_device):
    from diff_gaussian_rasterization import _native as N
    c, args, run = _case(N, "views3", gpu_device)
    ref = c["ref"]
    got = _contrib(N, args, run)
    R.check(got, ref, "V = 3")
    R.check_total(got["weight_sum"], ref, "V = 3")
    singles = []
    for v in range(3):
        a1 = _args(c["scenes"][v:v + 1], gpu_device)
        singles.append(_contrib(N, a1, _forward(N, a1)))
    assert np.array_equal(got["pixel_count"], sum(s["pixel_count"] for s in singles))
    assert np.array_equal(got["dominant_count"], sum(s["dominant_count"] for s in singles))
    assert got["weight_max"].tobytes() == np.maximum.reduce([s["weight_max"] for s in singles]).tobytes()
    three = sum(s["weight_sum"].astype(np.float64) for s in singles)
    assert (np.abs(got["weight_sum"] - three) <= 2 * R.sum_bar(ref, ref["sum"])).all()      # (both lie within the bar of the same value)
    # accumulate = 1 on the first call's results: doubled counts, the same maximum, the sum within the bar
    two = _contrib(N, args, run, old=got)
    assert np.array_equal(two["pixel_count"], 2 * got["pixel_count"]) and np.array_equal(two["dominant_count"], 2 * got["dominant_count"])
    assert two["weight_max"].tobytes() == got["weight_max"].tobytes()
    R.check(two, ref, "accumulate", old=got)
    # ... and over preset running values: a larger old maximum stays
    P = got["weight_sum"].shape[0]
    rng = np.random.default_rng(8)
    old = dict(weight_sum=rng.uniform(0, 50, P).astype(F), weight_max=rng.uniform(0, 0.6, P).astype(F),
               pixel_count=rng.integers(0, 1000, P).astype(np.int32), dominant_count=rng.integers(0, 100, P).astype(np.int32))
    acc = _contrib(N, args, run, old=old)
    R.check(acc, ref, "accumulate over preset values", old=old)
    assert (acc["weight_max"] == old["weight_max"]).any() and (acc["weight_max"] > old["weight_max"]).any()
    assert acc["weight_max"].tobytes() == np.maximum(old["weight_max"], got["weight_max"]).tobytes()


@pytest.mark.parametrize("name", R.WEIGHTED)
def test_pixel_weights(gpu_device, name):
    """a 0/1 mask with a whole quadrant zero; random weights with negatives and NaN, which count as 0"""
    from diff_gaussian_rasterization import _native as N
    c, args, run = _case(N, name, gpu_device)
    got = _contrib(N, args, run, weights=c["weights"])
    R.check(got, c["ref"], name)
    plain = _contrib(N, args, run)
    R.check(plain, R.case("views3")["ref"], name + " without the map")
    assert (got["pixel_count"] <= plain["pixel_count"]).all() and got["pixel_count"].sum() < plain["pixel_count"].sum()
    assert np.isfinite(got["weight_sum"]).all() and np.isfinite(got["weight_max"]).all()
    if name == "views3_mask":      # weights of 0 and 1: the maximum is one of the unweighted weights or smaller
        assert (got["weight_max"] <= plain["weight_max"]).all()
        cleaned = _contrib(N, args, run, weights=R.clean_map(c["weights"]))
        assert _bits(cleaned) == _bits(got)


@pytest.mark.parametrize("mode", ["colors", "sh", "cov3d"])
def test_random_scene_with_every_input_form(gpu_device, mode):
    """P = 2000 on 130 x 35: both colour sources (the statistics do not depend on the colours) and cov3D_precomp"""
    from diff_gaussian_rasterization import _native as N
    c = R.case("random2000", use_cov3d=mode == "cov3d")
    scenes = c["scenes"] if mode != "sh" else R.build("random2000", mode="sh")[0]
    args = _args(scenes, gpu_device)
    run = _forward(N, args)
    got = _contrib(N, args, run)
    R.check(got, c["ref"], mode)
    R.check_total(got["weight_sum"], c["ref"], mode)
    assert (got["pixel_count"] > 0).sum() > 1500


def _det_backward(N, args, run, dpix):
    return N.rasterize_gaussians_backward_batch(*colour_backward_args(args, run, dpix), deterministic=True)


def test_the_arenas_are_untouched(gpu_device):
    """need_backward forward, statistics, deterministic backward: the gradients of the same sequence without the statistics call, bit
    for bit -- and again after a recolor"""
    import util
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    c = R.case("views3")
    scs = c["scenes"]
    dpix = _t(np.stack([util.seeded_dL(s, seed=500 + v) for v, s in enumerate(scs)]), dev)
    cols = _t(np.random.default_rng(30).uniform(-0.2, 1.2, (3, scs[0].P, 3)).astype(F), dev)
    grads = {}
    for with_stats in (False, True):
        args = list(_args(scs, dev))
        run = _forward(N, args, need_backward=True)
        if with_stats:
            R.check(_contrib(N, args, run), c["ref"], "before the backward")
        grads[with_stats, "fwd"] = [g.cpu().numpy().tobytes() for g in _det_backward(N, args, run, dpix)]
        if with_stats:
            R.check(_contrib(N, args, run), c["ref"], "after the backward")
        N.recolor(args[0], args[1], cols, torch.empty(0), 0, args[16], scs[0].H, scs[0].W, run[0], run[3], run[4], run[5], need_backward=True)
        args[2] = cols
        if with_stats:
            R.check(_contrib(N, args, run), c["ref"], "after the recolor")
        grads[with_stats, "recolor"] = [g.cpu().numpy().tobytes() for g in _det_backward(N, args, run, dpix)]
    assert grads[True, "fwd"] == grads[False, "fwd"], "the statistics call changed what the backward reads"
    assert grads[True, "recolor"] == grads[False, "recolor"], "the statistics call changed what the backward after a recolor reads"
    assert grads[True, "fwd"] != grads[True, "recolor"]


def test_render_math_mode_does_not_matter_and_a_repeated_call_gives_the_same_bits(gpu_device):
    from diff_gaussian_rasterization import _native as N
    c, args, run = _case(N, "views3", gpu_device)
    got = _contrib(N, args, run)
    assert _bits(_contrib(N, args, run)) == _bits(got), "a repeated call returns other bits"
    old = N.get_render_math()
    N.set_render_math("fast")
    try:
        run_f = _forward(N, args)                       # (the forward itself now runs the fast kernels)
        fast = _contrib(N, args, run_f)
    finally:
        N.set_render_math(old)
    assert _bits(fast) == _bits(got), "the statistics depend on the render-math mode"
    R.check(fast, c["ref"], "fast render math")
    # the lane reduction kept for measurements (shuffle butterflies) adds the same pairs in the same tree
    import os
    os.environ["GSR_CONTRIB_REDUCE"] = "1"
    try:
        shuffled = _contrib(N, args, run)
    finally:
        del os.environ["GSR_CONTRIB_REDUCE"]
    assert _bits(shuffled) == _bits(got), "the two lane reductions disagree"
    R.check(shuffled, c["ref"], "shuffle reduction")


def test_a_mismatching_call_is_refused_with_the_outputs_untouched(gpu_device):
    from diff_gaussian_rasterization import _native as N
    c, args, run = _case(N, "views3", gpu_device)
    out = _prefilled(args[1].shape[0], gpu_device)
    with pytest.raises(RuntimeError, match=r"contrib_stats: V = 2, P = 400, 70 x 50, but the last forward or recolor .* had V = 3"):
        _contrib(N, args, run, V=2, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out[0]).all() and torch.isnan(out[1]).all() and (out[2] == SENTINEL).all() and (out[3] == SENTINEL).all()
    with pytest.raises(RuntimeError, match="all four outputs are NULL"):
        _contrib(N, args, run, want=())
    R.check(_contrib(N, args, run), c["ref"], "the matching call")


def test_rasterize_views_contrib(gpu_device):
    """images and radii are rasterize_views' bit for bit; stats is the C ABI's result; two calls accumulate"""
    import diff_gaussian_rasterization as d
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    c = R.case("views3_random")
    ref = c["ref"]
    scs = R.build("views3", mode="sh")[0]
    s = scs[0]
    P, V = s.P, len(scs)
    sts = _settings(scs, dev)
    m, o, sh, sc, ro = (_t(a, dev) for a in (s.means3D, s.opacities.reshape(-1, 1), s.shs, s.scales, s.rotations))
    m2 = torch.zeros_like(m)
    w = _t(c["weights"], dev)
    img_a, radii_a = d.rasterize_views(m, m2, o, sts, shs=sh, scales=sc, rotations=ro)
    stats = d.ContributionStats(P, dev)
    before = dict(N.CALLS)
    img_b, radii_b = d.rasterize_views_contrib(m.clone().requires_grad_(True), m2, o, sts, stats, pixel_weights=w, shs=sh, scales=sc,
                                               rotations=ro)
    assert N.CALLS["contrib_stats"] == before["contrib_stats"] + 1 and N.CALLS["backward"] == before["backward"]
    assert not img_b.requires_grad and torch.equal(img_a, img_b) and torch.equal(radii_a, radii_b)
    assert stats.pixels_seen == V * s.H * s.W
    got = {n: getattr(stats, n).cpu().numpy() for n in NAMES}
    R.check(got, ref, "through Python")
    args = _args(scs, dev)
    abi = _contrib(N, args, _forward(N, args), weights=c["weights"])
    assert _bits(abi) == _bits(got)
    assert (np.abs(abi["weight_sum"].astype(np.float64) - got["weight_sum"]) <= 2 * R.sum_bar(ref)).all()
    d.rasterize_views_contrib(m, m2, o, sts, stats, pixel_weights=w, shs=sh, scales=sc, rotations=ro)
    assert stats.pixels_seen == 2 * V * s.H * s.W
    assert np.array_equal(stats.pixel_count.cpu().numpy(), 2 * got["pixel_count"])
    R.check({n: getattr(stats, n).cpu().numpy() for n in NAMES}, ref, "second call", old=got)
    mw = stats.mean_weight().cpu().numpy()
    assert mw.shape == (P,) and np.isfinite(mw).all() and (mw[got["pixel_count"] > 0] > 0).all()
    with pytest.raises(Exception, match="stats was built for 7 Gaussians"):
        d.rasterize_views_contrib(m, m2, o, sts, d.ContributionStats(7, dev), shs=sh, scales=sc, rotations=ro)
    with pytest.raises(Exception, match="pixel_weights must be a float32 tensor"):
        d.rasterize_views_contrib(m, m2, o, sts, stats, pixel_weights=w.cpu(), shs=sh, scales=sc, rotations=ro)
    stats.reset()
    assert not stats.weight_sum.any() and stats.pixels_seen == 0
