"""The view-statistics entry (include/gsr.h gsr_backward_view_stats) as far as it can be reached without a GPU: the exported symbol,
the refusals that precede any HIP call, and the Python side -- DensityStats, rasterize_views_stats' validation and its refusal of CPU
tensors, pcrender.multiview.reduce_density_stats over gloo."""
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
A, B, Cc, D, E, Fp, G, Hh = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000   # stand-ins for device arrays (never followed)


def test_symbol_is_exported_declared_and_bound():
    from diff_gaussian_rasterization import _native as N
    sym = "gsr_backward_view_stats"
    assert hasattr(ctypes.CDLL(N.LIB_PATH), sym) and sym in N.SYMBOLS and sym in N._DECL
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+gsr_backward_view_stats\s*\(([^)]*)\)", header)
    assert m, "include/gsr.h does not declare %s" % sym
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(N._DECL[sym][1]) == 13
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "p", "V", "radii", "geom", "geom_bytes", "accumulate", "grad_norm_sum", "visible_views", "max_radius", "dL_dmean2D_views",
        "dL_dcolor_views", "dL_dopacity_views", "stream"]
    assert N.CALLS["backward_view_stats"] >= 0
    import diff_gaussian_rasterization as d
    assert list(inspect.signature(d.rasterize_views_stats).parameters) == [
        "means3D", "means2D", "opacities", "settings_list", "stats", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"]
    assert list(inspect.signature(d.DensityStats.__init__).parameters) == ["self", "P", "device", "keep_view_grads"]
    # the recolor paragraph no longer says that the per-view colour gradients cannot be had
    text = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "the per-view shares are not separated" not in text and "dL_dcolor_views" in text


def test_refusals_before_any_hip_call():
    from diff_gaussian_rasterization import _native as N
    call = N.lib.gsr_backward_view_stats

    def run(p, V=1, radii=A, geom=B, geom_bytes=1 << 20, accumulate=0, outs=(Cc, D, E, Fp, G, Hh)):
        return call(ctypes.byref(p), V, radii, geom, geom_bytes, accumulate, *outs, None), N.lib.gsr_last_error()

    assert call(None, 1, A, B, 0, 0, Cc, D, E, Fp, G, Hh, None) == -1 and b"params is NULL" in N.lib.gsr_last_error()
    rc, err = run(_params(N, W=0))
    assert rc == -1 and b"bad sizes" in err
    rc, err = run(_params(N, P=-1))
    assert rc == -1 and b"bad sizes" in err
    for V in (0, -1, 257):
        rc, err = run(_params(N), V=V)
        assert rc == -1 and b"view count" in err
    p = _params(N)
    p.viewmatrix = None
    rc, err = run(p)
    assert rc == -1 and b"required input pointer is NULL" in err
    # P == 0: nothing to do, success, whatever the pointers are
    assert run(_params(N, P=0), radii=None, geom=None, outs=(None,) * 6)[0] == 0
    assert run(_params(N, P=0), outs=(None, None, None, 0x1004, None, None))[0] == 0
    for kw in (dict(radii=None), dict(geom=None)):
        rc, err = run(_params(N), **kw)
        assert rc == -1 and b"backward_view_stats" in err and b"NULL" in err, (kw, err)
    # a NULL radii is reported before the outputs are looked at
    rc, err = run(_params(N), radii=None, outs=(None,) * 6)
    assert rc == -1 and b"required pointer is NULL" in err
    rc, err = run(_params(N), outs=(None,) * 6)
    assert rc == -1 and b"backward_view_stats" in err and b"nothing to write" in err
    for bad in (0x1004, 0x1001, 0x100C):
        rc, err = run(_params(N), outs=(Cc, D, E, bad, G, Hh))
        assert rc == -1 and b"dL_dmean2D_views is not 8-byte aligned" in err, err
    # only that output has an alignment of its own: a float-aligned one anywhere else gets as far as the size of the geometry
    # allocation (no arena has a record at this made-up address), the last check before the launch
    for outs in ((0x1004, None, None, None, None, None), (None, None, None, None, 0x1004, 0x100C), (Cc, D, E, Fp, G, Hh)):
        rc, err = run(_params(N), geom_bytes=16, outs=outs)
        assert rc == -3 and b"geom arena too small" in err, (outs, err)


def test_density_stats():
    import diff_gaussian_rasterization as d
    st = d.DensityStats(5, "cpu")
    assert st.P == 5 and st.device == torch.device("cpu") and st.keep_view_grads is False and st.view_grads is None
    for t, dt in ((st.grad_norm_sum, torch.float32), (st.visible_views, torch.int32), (st.max_radius, torch.int32)):
        assert tuple(t.shape) == (5,) and t.dtype == dt and t.device.type == "cpu" and t.is_contiguous() and not t.any()
    st.grad_norm_sum.copy_(torch.tensor([6.0, 0.0, 1.5, 9.0, 0.0]))
    st.visible_views.copy_(torch.tensor([3, 0, 1, 12, 0]))
    st.max_radius.fill_(7)
    m = st.mean_grad()
    assert m.dtype == torch.float32 and m.tolist() == [2.0, 0.0, 1.5, 0.75, 0.0]
    keep = (st.grad_norm_sum, st.visible_views, st.max_radius)
    st.view_grads = dict(mean2D=torch.zeros(2, 5, 2))
    st.reset()
    assert st.view_grads is None
    for t, k in zip((st.grad_norm_sum, st.visible_views, st.max_radius), keep):
        assert t is k and not t.any()             # in place: the tensors a trainer holds on to stay the accumulators
    st0 = d.DensityStats(0, "cpu", keep_view_grads=True)
    assert st0.keep_view_grads is True and st0.grad_norm_sum.shape == (0,) and st0.mean_grad().shape == (0,)


def test_rasterize_views_stats_validates_and_refuses_cpu_tensors():
    import diff_gaussian_rasterization as d
    from diff_gaussian_rasterization import _native as N
    m = torch.zeros(2, 3, requires_grad=True)
    st = _settings()
    stats = d.DensityStats(2, "cpu")
    ok = dict(colors_precomp=m, scales=m, rotations=torch.zeros(2, 4))
    with pytest.raises(Exception, match="empty settings list"):
        d.rasterize_views_stats(m, m, m[:, :1], [], stats, **ok)
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        d.rasterize_views_stats(m, m, m[:, :1], [st, st], stats)
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        d.rasterize_views_stats(m, m, m[:, :1], [st], stats, colors_precomp=m, scales=m)
    with pytest.raises(Exception, match="must be a DensityStats"):
        d.rasterize_views_stats(m, m, m[:, :1], [st], None, **ok)
    with pytest.raises(Exception, match="stats was built for 3 Gaussians on cpu, the cloud has 2 on cpu"):
        d.rasterize_views_stats(m, m, m[:, :1], [st], d.DensityStats(3, "cpu"), **ok)
    with pytest.raises(Exception, match="stats was built for 2 Gaussians on meta"):
        d.rasterize_views_stats(m, m, m[:, :1], [st], d.DensityStats(2, "meta"), **ok)
    with pytest.raises(Exception, match="must share image size"):
        d.rasterize_views_stats(m, m, m[:, :1], [st, st._replace(image_width=16)], stats, **ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.rasterize_views_stats(m, m, m[:, :1], [st, st], stats, **ok)
    assert not stats.grad_norm_sum.any() and not stats.visible_views.any() and not stats.max_radius.any() and stats.view_grads is None
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.backward_view_stats(torch.zeros(3), m.detach(), torch.zeros(2, 2, dtype=torch.int32), m.detach(), m.detach(), torch.zeros(2, 4),
                              1.0, torch.empty(0), torch.eye(4).repeat(2, 1, 1), torch.eye(4).repeat(2, 1, 1), 1.0, 1.0, 8, 8,
                              torch.empty(0), 0, torch.zeros(2, 3), torch.empty(0, dtype=torch.uint8),
                              grad_norm_sum=stats.grad_norm_sum)


# ---- reduce_density_stats over gloo ---------------------------------------------------------------------------------------------
def _rank_stats(rank, P=7):
    import diff_gaussian_rasterization as d
    st = d.DensityStats(P, "cpu")
    i = torch.arange(P)
    st.grad_norm_sum.copy_((i + 1).float() * 0.25 * (rank + 1))
    st.visible_views.copy_(((i + rank) % 4).int())
    st.max_radius.copy_(((i * 5 + rank * 3) % 11).int())
    return st


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pcrender import multiview
    try:
        st = _rank_stats(rank)
        keep = st.grad_norm_sum
        back = multiview.reduce_density_stats(st)
        parts = [_rank_stats(r) for r in range(world)]
        ok = back is st and st.grad_norm_sum is keep
        ok = ok and torch.equal(st.grad_norm_sum, torch.stack([p.grad_norm_sum for p in parts]).sum(0))     # (quarters: exact)
        ok = ok and torch.equal(st.visible_views, torch.stack([p.visible_views for p in parts]).sum(0).int())
        ok = ok and torch.equal(st.max_radius, torch.stack([p.max_radius for p in parts]).max(0).values)
        ok = ok and st.visible_views.dtype == torch.int32 and st.max_radius.dtype == torch.int32
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world, port", [(2, 29671), (3, 29672)])
def test_reduce_density_stats_over_gloo(world, port):
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


def test_reduce_density_stats_single_process_passthrough():
    from pcrender import multiview
    st = _rank_stats(1)
    want = _rank_stats(1)
    assert multiview.reduce_density_stats(st) is st
    assert torch.equal(st.grad_norm_sum, want.grad_norm_sum) and torch.equal(st.max_radius, want.max_radius)
