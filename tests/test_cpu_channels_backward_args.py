"""Argument checks of the channels backward's C entries that need no device (gsr_extra_state_bytes,
gsr_forward_batch_channels_train, gsr_backward_batch_channels)."""
import ctypes

import pytest


def _params(N, P=10):
    p = N.GsrParams()
    p.P, p.W, p.H = P, 64, 48
    # (dummy addresses: every check below fails before anything is read)
    p.means3D = p.opacities = p.bg = p.viewmatrix = p.projmatrix = p.campos = p.colors_precomp = p.scales = p.rotations = 0x1000
    return p


def _bwd(N, p, nx=8, layout=1, extra=1, state=1, dextra=1, out=1, bgx=1, geom=None):
    return N.lib.gsr_backward_batch_channels(ctypes.byref(p), 1, None, geom, 0, None, 0, None, 0, None, None, None, None, None, None,
                                             None, None, None, nx, layout, extra, None, bgx, state, 0, dextra, out, None)


def test_extra_state_bytes():
    from diff_gaussian_rasterization import _native as N
    lib = N.lib
    assert lib.gsr_extra_state_bytes(64, 48, 1000, 5) == 0
    assert lib.gsr_extra_state_bytes(0, 48, 1000, 4) == 0
    a4, a8 = lib.gsr_extra_state_bytes(1920, 1080, 10_000_000, 4), lib.gsr_extra_state_bytes(1920, 1080, 10_000_000, 8)
    # nx accumulated values per pixel + nx values per pixel and saved slice boundary (one per 512 list entries)
    assert 4 * 4 * 1920 * 1080 < a4 < a8 <= 2 * a4 + 256
    assert lib.gsr_extra_state_bytes(64, 48, 2_000_000, 8) > lib.gsr_extra_state_bytes(64, 48, 1_000, 8)


def test_channels_backward_rejects_bad_arguments_without_a_gpu():
    from diff_gaussian_rasterization import _native as N
    p = _params(N)
    rc = _bwd(N, p, nx=5)
    assert rc == -1 and b"4 or 8" in N.lib.gsr_last_error()
    rc = _bwd(N, p, nx=4, layout=2)
    assert rc == -1 and b"extra_per_view" in N.lib.gsr_last_error()
    rc = _bwd(N, p, extra=None)
    assert rc == -1 and b"NULL" in N.lib.gsr_last_error()
    rc = _bwd(N, p, state=None)
    assert rc == -1 and b"extra_state" in N.lib.gsr_last_error()
    # no forward ever ran on this (made-up) geometry arena
    rc = _bwd(N, p, geom=0x1000)
    assert rc == -1 and b"no forward on this geometry arena" in N.lib.gsr_last_error()


def test_channels_train_forward_rejects_bad_arguments_without_a_gpu():
    from diff_gaussian_rasterization import _native as N
    p = _params(N)
    R = (ctypes.c_int64 * 1)()
    rc = N.lib.gsr_forward_batch_channels_train(ctypes.byref(p), 1, None, 0, None, 0, None, 0, None, None, R, 0, 8, 1, 1, None, 1,
                                                1, None, 0, None)
    assert rc == -1 and b"extra_state is NULL" in N.lib.gsr_last_error()
    rc = N.lib.gsr_forward_batch_channels_train(ctypes.byref(p), 1, None, 0, None, 0, None, 0, None, None, R, 0, 3, 1, 1, None, 1,
                                                1, 1, 0, None)
    assert rc == -1 and b"4 or 8" in N.lib.gsr_last_error()


def test_python_entry_points_exist():
    import diff_gaussian_rasterization as d
    from pcrender import raster_passes as rp
    import inspect
    assert list(inspect.signature(d.rasterize_views_channels).parameters) == [
        "means3D", "means2D", "opacities", "settings_list", "extra", "bg_extra", "extra_view_scale", "shs", "colors_precomp", "scales",
        "rotations", "cov3D_precomp"]
    assert inspect.signature(rp.train_passes).parameters.keys() == inspect.signature(rp.render_passes).parameters.keys()
    with pytest.raises(Exception, match="empty settings list"):
        d.rasterize_views_channels(None, None, None, [], None, None)
