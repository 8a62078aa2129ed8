"""gsr_backward_view_stats (csrc/view_stats.hip) on the GPU: the three density-control statistics and the per-view shares after each
kind of backward, held to the host reference of tests/view_stats_ref.py fed with the library's own records (N.grad_records) and
radii -- integers exact, shares bit-equal, grad_norm_sum within 1 float32 ulp of the float64 value --, to the summing identities on the
backward's own outputs, and through the Python layer (rasterize_views_stats, DensityStats).  Every output is prefilled before every
call (NaN, or a sentinel for the integers): a row that is not written shows.  Images are 64 x 48."""
import itertools

import numpy as np
import pytest
import torch

import util
import view_stats_ref as R
from native_calls import (channels_backward_args, colour_backward_args, follower_args, scene_args as _args, scene_settings as _settings,
                          to_device as _t)

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -12345
NAMES = R.STATS + R.SHARES


def _forward(N, args, need_backward=True):
    counts, color, radii, geom, binning, img = N.rasterize_gaussians_batch(*args, need_backward=need_backward)
    return counts, color, radii, geom, binning, img


def _backward(N, args, run, dpix, deterministic=False):
    """the reference's 8-tuple: dL_dmeans2D [P,3], dL_dcolors [P,3], dL_dopacity [P,1], ..."""
    return N.rasterize_gaussians_backward_batch(*colour_backward_args(args, run, dpix), deterministic=deterministic)


def _prefilled(V, P, dev, old=None):
    """the six outputs: the statistics hold `old` (accumulate = 1) or garbage (accumulate = 0), the shares NaN"""
    if old is None:
        stats = [torch.full((P,), float("nan"), device=dev), torch.full((P,), SENTINEL, dtype=torch.int32, device=dev),
                 torch.full((P,), SENTINEL, dtype=torch.int32, device=dev)]
    else:
        stats = [_t(np.asarray(o), dev) for o in old]
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    return stats + [nan(V, P, 2), nan(V, P, 3), nan(V, P)]


def _stats(N, args, radii, geom, old=None, want=NAMES, V=None, out=None):
    """one gsr_backward_view_stats call for the outputs named in `want` (the others NULL): dict of numpy arrays"""
    dev = args[1].device
    V = args[8].shape[0] if V is None else V
    out = _prefilled(V, args[1].shape[0], dev, old) if out is None else out
    o = [t if n in want else None for n, t in zip(NAMES, out)]
    N.backward_view_stats(*follower_args(args, radii, geom, V), accumulate=old is not None, grad_norm_sum=o[0], visible_views=o[1],
                          max_radius=o[2], _out=tuple(o[3:]))
    return {n: t.cpu().numpy() for n, t in zip(NAMES, o) if t is not None}


def _records(N, geom, P, V):
    return np.stack([N.grad_records(geom, P, view=v, n_views=V).cpu().numpy() for v in range(V)])


def _bits(d):
    return b"".join(np.ascontiguousarray(d[n]).tobytes() for n in NAMES if n in d)


def _identities(got, g, tag):
    """adding the shares in float32 for v = 0, 1, .. from +0 gives the backward's summed outputs bit for bit"""
    for share, summed in (("mean2D", g[0][:, :2]), ("color", g[1]), ("opacity", g[2][:, 0])):
        acc = np.zeros(got[share].shape[1:], F)
        for v in range(got[share].shape[0]):
            acc = acc + got[share][v]
        want = summed.cpu().numpy()
        assert acc.dtype == F and acc.view(np.uint32).tolist() == want.view(np.uint32).tolist(), "%s: sum_v %s is not the backward's" % (tag, share)
        if got[share].shape[0] == 1:
            assert got[share][0].tobytes() == np.ascontiguousarray(want).tobytes(), (tag, share)


def _held(N, args, run, g, tag, old=None):
    """a full call against the reference fed from the arenas, plus the identities; returns (outputs, records, radii)"""
    P, V = args[1].shape[0], args[8].shape[0]
    radii = run[2].cpu().numpy()
    got = _stats(N, args, run[2], run[3], old=old)
    rec = _records(N, run[3], P, V)
    R.check(got, R.reference(rec, radii, old), tag)
    assert not (rec[radii <= 0][:, :9] != 0).any(), tag + ": a record of an invisible Gaussian is not zero"
    if g is not None:
        _identities(got, g, tag)
    return got, rec, radii


@pytest.mark.parametrize("V", [1, 2, 3, 12])
@pytest.mark.parametrize("P", [1, 63, 257, 1025])
def test_lane_wave_block_and_view_loop_edges(gpu_device, P, V):
    """one Gaussian; less than a wave; a block and one row; four blocks and one row -- with no group of four views, a remainder of
    one, two, three, and three whole groups"""
    from diff_gaussian_rasterization import _native as N
    scs = R.scenes(P, V)
    args = _args(scs, gpu_device)
    run = _forward(N, args)
    g = _backward(N, args, run, _t(np.stack(R.dLs(scs)), gpu_device))
    got, rec, radii = _held(N, args, run, g, "P=%d V=%d" % (P, V))
    if P >= 63:
        assert (got["visible_views"] > 0).any() and (got["grad_norm_sum"] > 0).any()
        assert got["max_radius"].max() == radii.max() > 0


def test_a_view_that_sees_nothing_and_a_cloud_partly_behind_the_camera(gpu_device):
    from diff_gaussian_rasterization import _native as N
    P = 257
    scs = R.scenes(P, 3, blind=True)
    args = _args(scs, gpu_device)
    run = _forward(N, args)
    g = _backward(N, args, run, _t(np.stack(R.dLs(scs)), gpu_device))
    got, rec, radii = _held(N, args, run, g, "blind view")
    assert run[0][1] == 0 and not (radii[1] > 0).any() and (radii[0] > 0).sum() > 100 and (radii[2] > 0).sum() > 100
    for n in R.SHARES:
        assert not got[n][1].view(np.uint32).any(), "the view that sees nothing must get +0 everywhere (%s)" % n
    assert got["visible_views"].max() == 2
    behind = np.arange(P)[5::13]          # behind cameras 0 and 1, in front of the opposite one
    assert not (radii[0, behind] > 0).any() and (radii[2, behind] > 0).any()
    seen = behind[radii[2, behind] > 0]
    assert (got["visible_views"][seen] == 1).all() and (got["max_radius"][seen] == radii[2, seen]).all()


WRITERS = ("atomic", "deterministic", "train_math", "channels", "recolor_per_view")


def _write(N, kind, scs, dev, dL_seed=500):
    """forward + the backward of `kind` on fresh arenas: (args, run, the backward's outputs)"""
    import camera_cases as CC
    args = list(_args(scs, dev))
    dpix = _t(np.stack(R.dLs(scs, seed=dL_seed)), dev)
    V, P = len(scs), scs[0].P
    if kind == "train_math":
        N.set_train_math(1)
        try:
            run = _forward(N, args)
            return args, run, _backward(N, args, run, dpix)
        finally:
            N.set_train_math(0)
    if kind == "channels":
        x, sc, bgx, dx = CC.channels_inputs(scs)
        extra = (_t(x, dev), _t(sc, dev), _t(bgx, dev))
        run = N.rasterize_gaussians_batch(*args, need_backward=True, extra=extra)
        g = N.rasterize_gaussians_backward_channels_batch(*channels_backward_args(args, run, dpix, extra, _t(dx, dev), 1.0))
        return args, run, g
    run = _forward(N, args)
    if kind == "recolor_per_view":
        cols = _t(np.random.default_rng(30).uniform(-0.2, 1.2, (V, P, 3)).astype(F), dev)
        e = torch.empty(0)
        N.recolor(args[0], args[1], cols, e, 0, args[16], R.H, R.W, run[0], run[3], run[4], run[5], need_backward=True)
        args[2], args[14], args[15] = cols, e, 0
    return args, run, _backward(N, args, run, dpix, deterministic=kind == "deterministic")


@pytest.mark.parametrize("kind", WRITERS)
def test_after_each_writer_of_the_records(gpu_device, kind):
    from diff_gaussian_rasterization import _native as N
    scs = R.scenes(1025, 3)
    args, run, g = _write(N, kind, scs, gpu_device)
    got, rec, radii = _held(N, args, run, g, kind)
    assert rec[:, :, 5:8].any() and rec[:, :, 8].any() and (got["visible_views"] == 3).any()
    again = _stats(N, args, run[2], run[3])
    assert _bits(again) == _bits(got), kind + ": a repeated call returns other bits"
    if kind == "deterministic":
        args2, run2, g2 = _write(N, kind, scs, gpu_device)
        assert _bits(_stats(N, args2, run2[2], run2[3])) == _bits(got), "two deterministic rounds differ"
    if kind == "channels":
        _, run_c, _ = _write(N, "atomic", scs, gpu_device)
        colour_only = _stats(N, args, run_c[2], run_c[3])
        assert (np.abs(colour_only["mean2D"] - got["mean2D"]).max() > 1e-3 * np.abs(got["mean2D"]).max()), "the extras' share did not arrive"
    if kind == "recolor_per_view":
        # the separation include/gsr.h used to say does not exist: view v's own colours' gradient
        assert all(got["color"][v].any() for v in range(3)) and got["color"][0].tobytes() != got["color"][1].tobytes()


def test_the_sum_of_the_norms_is_not_the_norm_of_the_sum(gpu_device):
    """opposite cameras: on the library's own records the two lie more than 1e-3 apart on at least a quarter of the Gaussians seen by
    two or more views (tests/test_cpu_view_stats_ref.py shows the same with the plain-C oracle), and the call returns the former"""
    from diff_gaussian_rasterization import _native as N
    scs = R.scenes(257, 3)
    args, run, g = _write(N, "atomic", scs, gpu_device)
    got, rec, radii = _held(N, args, run, g, "semantic point")
    rows, far = R.norm_gap(rec, radii)
    print("visible in >= 2 views: %d of 257; the two norms differ by > 1e-3 on %d" % (rows.sum(), far.sum()))
    assert rows.sum() >= 100 and 4 * far.sum() >= rows.sum()
    norm_of_sum = np.linalg.norm(g[0][:, :2].cpu().numpy().astype(np.float64), axis=1)
    assert (got["grad_norm_sum"][far] > norm_of_sum[far] * (1 + 5e-4)).all()


def test_every_subset_of_the_outputs(gpu_device):
    from diff_gaussian_rasterization import _native as N
    scs = R.scenes(257, 3)
    args, run, g = _write(N, "atomic", scs, gpu_device)
    full = _stats(N, args, run[2], run[3])
    for k in range(1, 6):
        for want in itertools.combinations(NAMES, k):
            part = _stats(N, args, run[2], run[3], want=want)
            assert tuple(part) == want
            for n in want:
                assert part[n].tobytes() == full[n].tobytes(), (want, n)
    # ... and the same under accumulate = 1: the shares are overwritten all the same
    old = (np.full(257, 0.5, F), np.full(257, 3, np.int32), np.full(257, 9, np.int32))
    full = _stats(N, args, run[2], run[3], old=old)
    for want in (("visible_views",), ("grad_norm_sum", "opacity"), ("max_radius", "mean2D", "color")):
        part = _stats(N, args, run[2], run[3], old=old, want=want)
        for n in want:
            assert part[n].tobytes() == full[n].tobytes(), (want, n)


def test_accumulate_over_preset_accumulators(gpu_device):
    from diff_gaussian_rasterization import _native as N
    P = 1025
    scs = R.scenes(P, 3)
    args, run, g = _write(N, "atomic", scs, gpu_device)
    rng = np.random.default_rng(8)
    rec, radii = _records(N, run[3], P, 3), run[2].cpu().numpy()
    scale = float(R.reference(rec, radii)["grad_norm_sum"].max())
    old = (rng.uniform(0, 4 * scale, P).astype(F), rng.integers(0, 1000, P).astype(np.int32), rng.integers(0, 2 * radii.max(), P).astype(np.int32))
    one, _, _ = _held(N, args, run, g, "accumulate once", old=old)
    ref1 = R.reference(rec, radii, old)
    assert (one["max_radius"] == old[2]).any() and (one["max_radius"] > old[2]).any()
    plain = R.reference(rec, radii)
    assert not np.array_equal(one["grad_norm_sum"], plain["grad_norm_sum"]) and not np.array_equal(one["visible_views"], plain["visible_views"])
    # the second call starts from the first one's float32 values: the reference applied to them, the integers the reference applied twice
    carry = (one["grad_norm_sum"], one["visible_views"], one["max_radius"])
    two = _stats(N, args, run[2], run[3], old=carry)
    R.check(two, R.reference(rec, radii, carry), "accumulate twice")
    ref2 = R.reference(rec, radii, (ref1["grad_norm_sum"], ref1["visible_views"], ref1["max_radius"]))
    assert np.array_equal(two["visible_views"], ref2["visible_views"]) and np.array_equal(two["max_radius"], ref2["max_radius"])
    # against the reference applied twice on its own: the first results lie at most 1 ulp apart, the same non-negative sum is added to
    # both (the result's ulp is no smaller than the old value's) and each is rounded once more: at most 2 ulps apart
    assert (util.ulp_diff(two["grad_norm_sum"], ref2["grad_norm_sum"]) <= 2).all()


def test_a_second_backward_rewrites_the_records(gpu_device):
    from diff_gaussian_rasterization import _native as N
    scs = R.scenes(257, 3)
    args, run, g = _write(N, "atomic", scs, gpu_device)
    first, rec1, _ = _held(N, args, run, g, "first backward")
    g2 = _backward(N, args, run, _t(np.stack(R.dLs(scs, seed=900)), gpu_device))
    second, rec2, _ = _held(N, args, run, g2, "second backward")
    assert rec1.tobytes() != rec2.tobytes() and first["grad_norm_sum"].tobytes() != second["grad_norm_sum"].tobytes()
    assert first["visible_views"].tobytes() == second["visible_views"].tobytes() and first["max_radius"].tobytes() == second["max_radius"].tobytes()


def test_refusals_that_need_a_record(gpu_device):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    P, V = 257, 3
    scs = R.scenes(P, V)
    args = _args(scs, dev)

    def refused(run, message, views=V):
        out = _prefilled(views, P, dev)
        with pytest.raises(RuntimeError, match=message):
            _stats(N, args, run[2], run[3], V=views, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(out[0]).all() and (out[1] == SENTINEL).all() and (out[2] == SENTINEL).all(), "a refused call wrote a statistic"
        for o in out[3:]:
            assert torch.isnan(o).all(), "a refused call wrote a share"

    run = _forward(N, args)
    refused(run, "backward_view_stats: no backward has run since the last forward or recolor")
    _backward(N, args, run, _t(np.stack(R.dLs(scs)), dev))
    refused(run, r"backward_view_stats: V = 2, P = %d, %d x %d, but the last forward or recolor .* had V = 3" % (P, R.W, R.H), views=2)
    _stats(N, args, run[2], run[3])                         # (the matching call goes through)
    run0 = _forward(N, args, need_backward=False)
    refused(run0, "backward_view_stats: the last forward on this geometry arena had need_backward = 0")
    # a float-aligned [V][P][2] block (one float into an allocation) on arenas whose record would let the call through
    buf = torch.full((V * P * 2 + 1,), float("nan"), device=dev)
    with pytest.raises(RuntimeError, match="dL_dmean2D_views is not 8-byte aligned"):
        _stats(N, args, run[2], run[3], want=("mean2D",), out=[None, None, None, buf[1:].view(V, P, 2), None, None])
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def _leaves(s, dev):
    out = [_t(a, dev).requires_grad_(True) for a in (s.means3D, s.opacities.reshape(-1, 1), s.shs, s.scales, s.rotations)]
    return out + [torch.zeros_like(out[0], requires_grad=True)]


def test_rasterize_views_stats(gpu_device):
    """images, radii and every input gradient are rasterize_views' bit for bit (under the deterministic backward, so that two
    backwards give the same bits); the accumulators after two training steps are the host reference fed with the library's own
    shares; each view's share is the means2D.grad of a single-view GaussianRasterizer call by the project's gradient bar"""
    import diff_gaussian_rasterization as d
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    P, V = 1025, 3
    scs = R.scenes(P, V)
    s = scs[0]
    sts = _settings(scs, dev)
    steps = [_t(np.stack(R.dLs(scs, seed=seed)), dev) for seed in (500, 900)]
    old = N.get_deterministic()
    N.set_deterministic(True)
    try:
        stats = d.DensityStats(P, dev, keep_view_grads=True)
        want_stats = None
        for step, dL in enumerate(steps):
            m, o, sh, sc, ro, m2 = _leaves(s, dev)
            img_a, radii_a = d.rasterize_views(m, m2, o, sts, shs=sh, scales=sc, rotations=ro)
            (img_a * dL).sum().backward()
            want = [t.grad.clone() for t in (m, o, sh, sc, ro, m2)]

            m, o, sh, sc, ro, m2 = _leaves(s, dev)
            before = dict(N.CALLS)
            img_b, radii_b = d.rasterize_views_stats(m, m2, o, sts, stats, shs=sh, scales=sc, rotations=ro)
            assert stats.view_grads is None or step == 1                 # nothing happens before the backward
            (img_b * dL).sum().backward()
            assert N.CALLS["backward_view_stats"] == before["backward_view_stats"] + 1
            assert N.CALLS["backward_det"] == before["backward_det"] + 1 and N.CALLS["backward"] == before["backward"]
            assert torch.equal(img_a, img_b) and torch.equal(radii_a, radii_b)
            for w, t in zip(want, (m, o, sh, sc, ro, m2)):
                assert w.cpu().numpy().tobytes() == t.grad.cpu().numpy().tobytes()

            vg = {k: t.cpu().numpy() for k, t in stats.view_grads.items()}
            assert vg["mean2D"].shape == (V, P, 2) and vg["color"].shape == (V, P, 3) and vg["opacity"].shape == (V, P)
            acc = np.zeros((P, 2), F)
            for v in range(V):
                acc = acc + vg["mean2D"][v]
            assert acc.tobytes() == m2.grad[:, :2].contiguous().cpu().numpy().tobytes()
            # the host reference fed with the library's own shares
            rec = np.zeros((V, P, 16), F)
            rec[:, :, 0:2], rec[:, :, 5:8], rec[:, :, 8] = vg["mean2D"], vg["color"], vg["opacity"]
            ref = R.reference(rec, radii_b.cpu().numpy(), want_stats)
            got = dict(grad_norm_sum=stats.grad_norm_sum.cpu().numpy(), visible_views=stats.visible_views.cpu().numpy(),
                       max_radius=stats.max_radius.cpu().numpy())
            R.check(got, ref, "training step %d" % step)
            want_stats = (got["grad_norm_sum"], got["visible_views"], got["max_radius"])
        assert (stats.visible_views.cpu().numpy() == 2 * (radii_b.cpu().numpy() > 0).sum(0)).all()
        mg = stats.mean_grad().cpu().numpy()
        assert mg.shape == (P,) and np.isfinite(mg).all() and (mg[got["visible_views"] > 0] > 0).any()

        # each view's share against a single-view call of that view (slice lengths differ between V = 1 and a batch: the bar, not bits)
        for v in range(V):
            m, o, sh, sc, ro, m2 = _leaves(s, dev)
            img, _ = d.GaussianRasterizer(sts[v])(means3D=m, means2D=m2, opacities=o, shs=sh, scales=sc, rotations=ro)
            (img * steps[1][v]).sum().backward()
            util.check_grads(dict(dL_dmean2D=vg["mean2D"][v]), dict(dL_dmean2D=m2.grad[:, :2].cpu().numpy()), "view %d" % v,
                             names=("dL_dmean2D",))

        # no input needs a gradient: no backward, no extra call, stats as they are
        keep = stats.grad_norm_sum.clone()
        before = N.CALLS["backward_view_stats"]
        det = [t.detach() for t in _leaves(s, dev)]
        img_c, _ = d.rasterize_views_stats(det[0], det[5], det[1], sts, stats, shs=det[2], scales=det[3], rotations=det[4])
        assert N.CALLS["backward_view_stats"] == before and torch.equal(stats.grad_norm_sum, keep) and torch.equal(img_c, img_a)
        with pytest.raises(Exception, match="stats was built for 7 Gaussians"):
            d.rasterize_views_stats(m, m2, o, sts, d.DensityStats(7, dev), shs=sh, scales=sc, rotations=ro)
        stats.reset()
        assert not stats.grad_norm_sum.any() and stats.view_grads is None
    finally:
        N.set_deterministic(old)
