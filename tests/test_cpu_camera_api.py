"""The camera-gradient entry (include/gsr.h gsr_backward_cameras) as far as it can be reached without a GPU: the exported symbols,
the scratch-size query, the refusals that precede any HIP call, and the Python side (rasterize_views_cameras refuses CPU tensors;
pcrender.camera.raster_settings_tensors equals raster_settings_batch bit for bit and keeps the poses in the autograd graph)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from native_calls import unit_settings as _settings
from refusal_tables import follower_params as _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, Cc, D, E, Fp = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000   # stand-ins for device arrays (never followed)


def test_symbols_are_exported_and_bound():
    from diff_gaussian_rasterization import _native as N
    lib = ctypes.CDLL(N.LIB_PATH)
    for sym in ("gsr_camera_grad_bytes", "gsr_backward_cameras"):
        assert hasattr(lib, sym) and sym in N.SYMBOLS
    assert N.CALLS["backward_cameras"] >= 0
    import diff_gaussian_rasterization as d
    import inspect
    assert list(inspect.signature(d.rasterize_views_cameras).parameters) == [
        "means3D", "means2D", "opacities", "settings_list", "viewmatrices", "projmatrices", "campos", "shs", "colors_precomp",
        "scales", "rotations", "cov3D_precomp"]


def test_camera_grad_bytes():
    from diff_gaussian_rasterization import _native as N
    f = N.lib.gsr_camera_grad_bytes
    for V, P in ((0, 10), (-1, 10), (257, 10), (1, -1)):
        assert f(V, P) == 0, (V, P)
    sizes_p = (0, 1, 1023, 1024, 1025, 2051, 800_000, 2_000_000)
    for V in (1, 2, 12, 256):
        prev = 0
        for P in sizes_p:
            b = f(V, P)
            assert b > 0 and b % 256 == 0 and b >= prev, (V, P, b)
            prev = b
    for P in sizes_p:
        prev = 0
        for V in range(1, 257, 15):
            b = f(V, P)
            assert b >= prev, (V, P)
            prev = b
    # 256 B per 1024 Gaussians and view: 200 KB per view for 800 K Gaussians
    assert 12 * 782 * 256 <= f(12, 800_000) <= 12 * 782 * 256 + 512


def test_refusals_before_any_hip_call():
    from diff_gaussian_rasterization import _native as N
    call = N.lib.gsr_backward_cameras

    def run(p, V=1, radii=A, geom=B, geom_bytes=1 << 20, dv=Cc, dp=D, dc=E, scratch=Fp, scratch_bytes=None):
        if scratch_bytes is None:
            scratch_bytes = N.lib.gsr_camera_grad_bytes(V, max(p.P, 0))
        return call(ctypes.byref(p), V, radii, geom, geom_bytes, dv, dp, dc, scratch, scratch_bytes, None), N.lib.gsr_last_error()

    assert call(None, 1, A, B, 0, Cc, D, E, Fp, 0, None) == -1 and b"params is NULL" in N.lib.gsr_last_error()
    rc, err = run(_params(N, W=0))
    assert rc == -1 and b"bad sizes" in err
    rc, err = run(_params(N, P=-1))
    assert rc == -1 and b"bad sizes" in err
    for V in (0, 257):
        rc, err = run(_params(N), V=V, scratch_bytes=0)
        assert rc == -1 and b"view count" in err
    p = _params(N)
    p.viewmatrix = None
    rc, err = run(p)
    assert rc == -1 and b"required input pointer is NULL" in err
    # P == 0: nothing to do, success, whatever the pointers are
    assert run(_params(N, P=0), radii=None, geom=None, dv=None, dp=None, dc=None, scratch=None, scratch_bytes=0)[0] == 0
    for kw in (dict(radii=None), dict(geom=None), dict(dv=None), dict(dp=None), dict(dc=None), dict(scratch=None)):
        rc, err = run(_params(N), **kw)
        assert rc == -1 and b"backward_cameras" in err and b"NULL" in err, (kw, err)
    for V, P in ((1, 10), (3, 2051)):
        need = N.lib.gsr_camera_grad_bytes(V, P)
        rc, err = run(_params(N, P=P), V=V, scratch_bytes=need - 1)
        assert rc == -3 and re.search(rb"< %d\b" % need, err), err
    # a NULL pointer is reported before the scratch size
    rc, err = run(_params(N), dv=None, scratch_bytes=0)
    assert rc == -1 and b"NULL" in err


def test_rasterize_views_cameras_validates_and_refuses_cpu_tensors():
    import diff_gaussian_rasterization as d
    m = torch.zeros(2, 3)
    st = _settings()
    view, proj, cam = torch.eye(4).repeat(2, 1, 1).requires_grad_(True), torch.eye(4).repeat(2, 1, 1), torch.zeros(2, 3)
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        d.rasterize_views_cameras(m, m, m[:, :1], [st, st], view, proj, cam)
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        d.rasterize_views_cameras(m, m, m[:, :1], [st, st], view, proj, cam, colors_precomp=m, scales=m)
    with pytest.raises(Exception, match=r"\[V,4,4\]"):
        d.rasterize_views_cameras(m, m, m[:, :1], [st], view, proj, cam, colors_precomp=m, scales=m, rotations=torch.zeros(2, 4))
    with pytest.raises(Exception, match="must share image size"):
        d.rasterize_views_cameras(m, m, m[:, :1], [st, st._replace(image_width=16)], view, proj, cam, colors_precomp=m, scales=m,
                                  rotations=torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.rasterize_views_cameras(m, m, m[:, :1], [st, st], view, proj, cam, colors_precomp=m, scales=m, rotations=torch.zeros(2, 4))
    from diff_gaussian_rasterization import _native as N
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.backward_cameras(torch.zeros(3), m, torch.zeros(2, 2, dtype=torch.int32), m, m, torch.zeros(2, 4), 1.0, torch.empty(0), view,
                           proj, 1.0, 1.0, 8, 8, torch.empty(0), 0, cam, torch.empty(0, dtype=torch.uint8))


def test_raster_settings_tensors_equals_raster_settings_batch_bit_for_bit():
    from pcrender import camera
    g = np.load(os.path.join(ROOT, "tests", "golden", "py_camera.npz"))
    for tag in ("native", "hd", "fov60"):
        w, h, fov, ss = g[tag + "_args"]
        H = torch.from_numpy(g[tag + "_H_c2w"][0])
        a = camera.raster_settings_batch(H, int(w), int(h), float(fov), int(ss))
        b = camera.raster_settings_tensors(H, int(w), int(h), float(fov), int(ss))
        assert set(a) == set(b)
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].numpy().tobytes() == b[k].numpy().tobytes(), (tag, k)
            else:
                assert a[k] == b[k], (tag, k)
        assert b["viewmatrix"].numpy().tobytes() == g[tag + "_viewmatrix"].tobytes()      # ... and the reference's own values


def test_gradients_flow_to_the_poses():
    from pcrender import camera
    H = camera.circle_path(3, 0, 3, [90, 0]).double().requires_grad_(True)
    a = camera.raster_settings_tensors(H, 64, 48, 45.0, 2)
    assert a["viewmatrix"].requires_grad and a["projmatrix"].requires_grad and a["campos"].requires_grad
    assert a["viewmatrix"].dtype == torch.float64 and a["viewmatrix"].device == H.device

    def f(Hc):
        r = camera.raster_settings_tensors(Hc, 64, 48, 45.0, 2)
        return r["viewmatrix"], r["projmatrix"], r["campos"]

    assert torch.autograd.gradcheck(f, (H,), eps=1e-6, atol=1e-7)
