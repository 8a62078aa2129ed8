"""The contribution-statistics entry (include/gsr.h gsr_contrib_stats) as far as it can be reached without a GPU: the exported symbol,
the refusals that precede any HIP call, in their order, and the Python side -- ContributionStats, rasterize_views_contrib's validation
and its refusal of CPU tensors, pcrender.multiview.reduce_contribution_stats over gloo."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from native_calls import unit_settings as _settings
from refusal_tables import follower_params as _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, Cc, D, E, Fp, G, Hh, I = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000   # stand-ins for device arrays (never followed)
SYM = "gsr_contrib_stats"


def test_symbol_is_exported_declared_and_bound():
    from diff_gaussian_rasterization import _native as N
    assert hasattr(ctypes.CDLL(N.LIB_PATH), SYM) and SYM in N.SYMBOLS and SYM in N._DECL
    text = open(os.path.join(ROOT, "include", "gsr.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+gsr_contrib_stats\s*\(([^)]*)\)", header)
    assert m, "include/gsr.h does not declare %s" % SYM
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(N._DECL[SYM][1]) == 16
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "p", "V", "radii", "geom", "geom_bytes", "binning", "binning_bytes", "image", "image_bytes", "pixel_weights", "accumulate",
        "weight_sum", "weight_max", "pixel_count", "dominant_count", "stream"]
    assert N.CALLS["contrib_stats"] >= 0
    # the header says which outputs are bit-reproducible and that the arithmetic is the exact mode's
    doc = text[text.index("Per-Gaussian contribution statistics"):text.index("int gsr_contrib_stats")]
    assert "bit-reproducible" in doc and "weight_sum is NOT" in doc and "gsr_set_render_math" in doc and "gsr_set_train_math" in doc
    import diff_gaussian_rasterization as d
    assert list(inspect.signature(d.rasterize_views_contrib).parameters) == [
        "means3D", "means2D", "opacities", "settings_list", "stats", "pixel_weights", "shs", "colors_precomp", "scales", "rotations",
        "cov3D_precomp"]
    assert list(inspect.signature(d.ContributionStats.__init__).parameters) == ["self", "P", "device"]
    from pcrender import multiview
    assert list(inspect.signature(multiview.reduce_contribution_stats).parameters) == ["stats", "group"]


def test_refusals_before_any_hip_call_in_their_order():
    from diff_gaussian_rasterization import _native as N
    call = N.lib.gsr_contrib_stats
    BIG = 1 << 30

    def run(p, V=1, radii=A, geom=B, geom_bytes=BIG, binning=Cc, binning_bytes=BIG, image=D, image_bytes=BIG, weights=None,
            accumulate=0, outs=(E, Fp, G, Hh)):
        return (call(ctypes.byref(p), V, radii, geom, geom_bytes, binning, binning_bytes, image, image_bytes, weights, accumulate,
                     *outs, None), N.lib.gsr_last_error())

    # 1. the parameters, as every entry
    assert call(None, 1, A, B, 0, Cc, 0, D, 0, None, 0, E, Fp, G, Hh, None) == -1 and b"params is NULL" in N.lib.gsr_last_error()
    rc, err = run(_params(N, W=0))
    assert rc == -1 and b"bad sizes" in err
    rc, err = run(_params(N, P=-1))
    assert rc == -1 and b"bad sizes" in err
    for V in (0, -1, 257):
        rc, err = run(_params(N), V=V, geom=None, outs=(None,) * 4)      # ... before anything else is looked at
        assert rc == -1 and b"view count" in err
    p = _params(N)
    p.viewmatrix = None
    rc, err = run(p)
    assert rc == -1 and b"required input pointer is NULL" in err
    # 2. P == 0: nothing to do, success, whatever the pointers are
    assert run(_params(N, P=0), radii=None, geom=None, binning=None, image=None, outs=(None,) * 4)[0] == 0
    assert run(_params(N, P=0), geom_bytes=0, binning_bytes=0, image_bytes=0)[0] == 0
    # 3. a NULL arena, before the outputs are looked at; radii may be NULL
    for kw in (dict(geom=None), dict(binning=None), dict(image=None)):
        for outs in ((E, Fp, G, Hh), (None,) * 4):
            rc, err = run(_params(N), outs=outs, **kw)
            assert rc == -1 and b"contrib_stats: a required pointer is NULL" in err, (kw, err)
    # 4. all four outputs NULL
    rc, err = run(_params(N), outs=(None,) * 4, geom_bytes=16)
    assert rc == -1 and b"contrib_stats" in err and b"all four outputs are NULL" in err
    # 5. (the arena's record: no arena has one at this made-up address)  6. the arena sizes, geometry first; any subset of the
    # outputs, a weight map and a NULL radii get that far
    for outs in ((E, None, None, None), (None, Fp, None, None), (None, None, G, None), (None, None, None, Hh), (E, Fp, G, Hh)):
        for radii, weights in ((A, None), (None, I)):
            rc, err = run(_params(N), radii=radii, weights=weights, geom_bytes=16, outs=outs)
            assert rc == -3 and b"geom arena too small" in err and b"need_backward" not in err, (outs, err)
    need = N.lib.gsr_geom_bytes_inference(10)
    rc, err = run(_params(N), geom_bytes=need, image_bytes=16)
    assert rc == -3 and b"image arena too small" in err
    rc, err = run(_params(N), geom_bytes=need, image_bytes=BIG, binning_bytes=16)
    assert rc == -3 and b"binning arena too small" in err


def test_contribution_stats():
    import diff_gaussian_rasterization as d
    st = d.ContributionStats(5, "cpu")
    assert st.P == 5 and st.device == torch.device("cpu") and st.pixels_seen == 0 and type(st.pixels_seen) is int
    fields = ((st.weight_sum, torch.float32), (st.weight_max, torch.float32), (st.pixel_count, torch.int32), (st.dominant_count, torch.int32))
    for t, dt in fields:
        assert tuple(t.shape) == (5,) and t.dtype == dt and t.device.type == "cpu" and t.is_contiguous() and not t.any()
    st.weight_sum.copy_(torch.tensor([6.0, 0.0, 1.5, 9.0, 0.0]))
    st.pixel_count.copy_(torch.tensor([3, 0, 1, 12, 0]))
    st.weight_max.fill_(0.5)
    st.dominant_count.fill_(2)
    st.pixels_seen = 640
    m = st.mean_weight()
    assert m.dtype == torch.float32 and m.tolist() == [2.0, 0.0, 1.5, 0.75, 0.0]
    st.reset()
    assert st.pixels_seen == 0
    for (t, _), k in zip(fields, (st.weight_sum, st.weight_max, st.pixel_count, st.dominant_count)):
        assert t is k and not t.any()             # in place: the tensors a caller holds on to stay the accumulators
    st0 = d.ContributionStats(0, "cpu")
    assert st0.weight_sum.shape == (0,) and st0.mean_weight().shape == (0,)


def test_rasterize_views_contrib_validates_and_refuses_cpu_tensors():
    import diff_gaussian_rasterization as d
    from diff_gaussian_rasterization import _native as N
    m = torch.zeros(2, 3)
    st = _settings()
    stats = d.ContributionStats(2, "cpu")
    ok = dict(colors_precomp=m, scales=m, rotations=torch.zeros(2, 4))
    with pytest.raises(Exception, match="empty settings list"):
        d.rasterize_views_contrib(m, m, m[:, :1], [], stats, **ok)
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        d.rasterize_views_contrib(m, m, m[:, :1], [st, st], stats)
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        d.rasterize_views_contrib(m, m, m[:, :1], [st], stats, colors_precomp=m, scales=m)
    with pytest.raises(Exception, match="must be a ContributionStats"):
        d.rasterize_views_contrib(m, m, m[:, :1], [st], None, **ok)
    with pytest.raises(Exception, match="must be a ContributionStats"):
        d.rasterize_views_contrib(m, m, m[:, :1], [st], d.DensityStats(2, "cpu"), **ok)
    with pytest.raises(Exception, match="stats was built for 3 Gaussians on cpu, the cloud has 2 on cpu"):
        d.rasterize_views_contrib(m, m, m[:, :1], [st], d.ContributionStats(3, "cpu"), **ok)
    with pytest.raises(Exception, match="stats was built for 2 Gaussians on meta"):
        d.rasterize_views_contrib(m, m, m[:, :1], [st], d.ContributionStats(2, "meta"), **ok)
    for bad in (torch.zeros(2, 8, 8, dtype=torch.float64), torch.zeros(1, 8, 8), torch.zeros(2, 8, 9), torch.zeros(2, 8, 8, device="meta"),
                [[1.0]]):
        with pytest.raises(Exception, match=r"pixel_weights must be a float32 tensor of shape \[2, 8, 8\] on cpu"):
            d.rasterize_views_contrib(m, m, m[:, :1], [st, st], stats, pixel_weights=bad, **ok)
    with pytest.raises(Exception, match="must share image size"):
        d.rasterize_views_contrib(m, m, m[:, :1], [st, st._replace(image_width=16)], stats, **ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.rasterize_views_contrib(m, m, m[:, :1], [st, st], stats, pixel_weights=torch.ones(2, 8, 8), **ok)
    assert not stats.weight_sum.any() and not stats.pixel_count.any() and stats.pixels_seen == 0
    e, u8 = torch.empty(0), torch.empty(0, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.contrib_stats(torch.zeros(3), m, torch.zeros(2, 2, dtype=torch.int32), m, m, torch.zeros(2, 4), 1.0, e,
                        torch.eye(4).repeat(2, 1, 1), torch.eye(4).repeat(2, 1, 1), 1.0, 1.0, 8, 8, e, 0, torch.zeros(2, 3), u8, u8, u8,
                        weight_sum=stats.weight_sum)


# ---- reduce_contribution_stats over gloo ----------------------------------------------------------------------------------------
def _rank_stats(rank, P=7):
    import diff_gaussian_rasterization as d
    st = d.ContributionStats(P, "cpu")
    i = torch.arange(P)
    st.weight_sum.copy_((i + 1).float() * 0.25 * (rank + 1))
    st.weight_max.copy_(((i * 3 + rank * 5) % 8).float() / 8)
    st.pixel_count.copy_(((i + rank) % 4).int())
    st.dominant_count.copy_(((i * 5 + rank * 3) % 11).int())
    st.pixels_seen = 1000 * (rank + 1) + 7
    return st


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pcrender import multiview
    try:
        st = _rank_stats(rank)
        keep = st.weight_sum
        back = multiview.reduce_contribution_stats(st)
        parts = [_rank_stats(r) for r in range(world)]
        ok = back is st and st.weight_sum is keep
        ok = ok and torch.equal(st.weight_sum, torch.stack([p.weight_sum for p in parts]).sum(0))     # (quarters: exact)
        ok = ok and torch.equal(st.weight_max, torch.stack([p.weight_max for p in parts]).max(0).values)
        ok = ok and torch.equal(st.pixel_count, torch.stack([p.pixel_count for p in parts]).sum(0).int())
        ok = ok and torch.equal(st.dominant_count, torch.stack([p.dominant_count for p in parts]).sum(0).int())
        ok = ok and st.pixel_count.dtype == torch.int32 and st.dominant_count.dtype == torch.int32
        ok = ok and type(st.pixels_seen) is int and st.pixels_seen == sum(p.pixels_seen for p in parts)
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_reduce_contribution_stats_over_gloo():
    world, port = 2, 29681
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(res) == [(r, True) for r in range(world)]


def test_reduce_contribution_stats_single_process_passthrough():
    from pcrender import multiview
    st = _rank_stats(1)
    want = _rank_stats(1)
    assert multiview.reduce_contribution_stats(st) is st
    assert torch.equal(st.weight_sum, want.weight_sum) and torch.equal(st.weight_max, want.weight_max)
    assert st.pixels_seen == want.pixels_seen
