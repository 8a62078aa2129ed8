"""Point-cloud neighbourhoods on the device (gsr_knn / gsr_cloud_geometry, pcrender.cloud) against the host references of cloud_ref on
the shared cases: the wave-run and coarse-box edges, the list lengths' own edges, lattices, repeats, one point many times, a line, a
cluster with far outliers, a large common exponent and absent points.

  knn        idx and d2 equal the float32 brute force exactly (the definition leaves no freedom: ties go to the lower index), the outputs
             between guard words; d2 = NULL, a points view 4 B off its 16-B boundary, a second call and a scratch prefilled with garbage
             give the same bits.
  geometry   on the device's lists and on hand-made lists every output is bit-identical to the float32 restatement, and each output
             asked for alone equals the same output of the full call.
  no device -> host copy is made by any of it (gsr_d2h_count).
  end to end a noisy sphere through gaussians_from_points in both modes, render_passes with its normals, and three GaussianAdam steps.
The reference lists are built once per case (cloud_ref.case_lists)."""
import numpy as np
import pytest
import torch

import cloud_ref as R
import native_calls as NC

pytestmark = pytest.mark.gpu
GUARD = 0x7FC0DEAD                                                            # a NaN pattern no kernel produces
PAD = 8
IDS = [c.name for c in R.CASES]


@pytest.fixture(scope="module")
def N():
    from diff_gaussian_rasterization import _native
    return _native


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(n, dev, dtype):
    big = torch.full((2 * PAD + n,), GUARD, dtype=torch.int32, device=dev)
    return big, big[PAD:PAD + n].view(dtype)


def _guards_hold(big, n):
    return bool((big[:PAD] == GUARD).all()) and bool((big[PAD + n:] == GUARD).all())


def _points(p, dev, shift=0):
    """the cloud on the device, `shift` floats off a 16-B boundary"""
    big = torch.zeros((p.size + 4 + shift,), dtype=torch.float32, device=dev)
    off = (-(big.data_ptr() // 4) % 4 + shift)
    view = big[off:off + p.size].view(-1, 3)
    view.copy_(NC.to_device(p, dev))
    assert (view.data_ptr() % 16 == 0) == (shift % 4 == 0)
    return view


def _knn(N, dev, pts, K, want_d2=True, fill=None):
    """the C ABI itself on guarded outputs and a scratch of the caller's; returns numpy (idx, d2 or None)"""
    P = pts.shape[0]
    big_i, idx = _guarded(P * K, dev, torch.int32)
    big_d, d2 = _guarded(P * K, dev, torch.float32)
    nbytes = N.lib.gsr_knn_scratch_bytes(P, K)
    assert nbytes > 0 and nbytes % 256 == 0
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if fill is not None:
        scratch.fill_(fill)
    before = N.lib.gsr_d2h_count()
    rc = N.lib.gsr_knn(P, pts.data_ptr(), K, idx.data_ptr(), d2.data_ptr() if want_d2 else None, scratch.data_ptr(), nbytes,
                       torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, N.lib.gsr_last_error()
    assert N.lib.gsr_d2h_count() == before
    torch.cuda.synchronize(dev)
    assert _guards_hold(big_i, P * K) and _guards_hold(big_d, P * K)
    if not want_d2:
        assert bool((big_d == GUARD).all())
    return idx.view(P, K).cpu().numpy(), d2.view(P, K).cpu().numpy() if want_d2 else None


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_knn_equals_the_brute_force(N, dev, c, K):
    p, want_idx, want_d2 = R.case_lists(c)
    idx, d2 = _knn(N, dev, _points(p, dev), K)
    wrong = np.flatnonzero((idx != want_idx[:, :K]).any(1))
    assert wrong.size == 0, (c.name, K, wrong[:5], idx[wrong[:2]], want_idx[wrong[:2], :K])
    assert np.array_equal(_bits(d2), _bits(want_d2[:, :K])), (c.name, K)
    # the padding is where the definition puts it
    avail = max(int(R.present_mask(p).sum()) - 1, 0)
    rows = R.present_mask(p)
    assert (idx[~rows] == -1).all() and np.isinf(d2[~rows]).all()
    assert (idx[rows][:, min(avail, K):] == -1).all() and (idx[rows][:, :min(avail, K)] >= 0).all()


@pytest.mark.parametrize("k", range(len(R.CASES)), ids=IDS)
def test_knn_bits_do_not_depend_on_d2_alignment_scratch_or_the_call(N, dev, k):
    c, K = R.CASES[k], R.KS[k % len(R.KS)]
    p = R.case_lists(c)[0]
    idx, d2 = _knn(N, dev, _points(p, dev), K, fill=0)
    for kw, shift in ((dict(want_d2=False), 0), (dict(), 1), (dict(), 0), (dict(fill=0xFF), 0), (dict(fill=0x5A), 3)):
        i2, dd = _knn(N, dev, _points(p, dev, shift), K, **kw)
        assert np.array_equal(i2, idx), (c.name, K, kw, shift)
        assert dd is None or np.array_equal(_bits(dd), _bits(d2)), (c.name, K, kw, shift)


def _geometry(N, dev, pts, idx_t, k_s, k_n, orient_to, want):
    before = N.lib.gsr_d2h_count()
    out = N.cloud_geometry(pts, idx_t, k_s=k_s, k_n=k_n, orient_to=orient_to, want=want)
    assert N.lib.gsr_d2h_count() == before
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_geometry(N, dev, p, idx, k_s, k_n, orient_to, tag):
    pts, idx_t = _points(p, dev), NC.to_device(idx, dev)
    ref = R.geometry(p, idx, k_s=k_s, k_n=k_n, orient_to=orient_to)
    full = _geometry(N, dev, pts, idx_t, k_s, k_n, orient_to, N.CLOUD_OUTPUTS)
    for name in N.CLOUD_OUTPUTS:
        want, got = getattr(ref, name), full[name]
        assert not np.isnan(got).any(), (tag, name)
        bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(len(p), -1).any(1))
        assert bad.size == 0, (tag, name, bad[:5], got[bad[:2]], want[bad[:2]])
        alone = _geometry(N, dev, pts, idx_t, k_s, k_n, orient_to, (name,))
        assert list(alone) == [name] and np.array_equal(_bits(alone[name]), _bits(got)), (tag, name)
    deg = ref.degenerate
    assert (full["cov6"][deg] == 0).all() and (full["normals"][deg] == [0, 0, 1]).all() and (full["rotations"][deg] == [1, 0, 0, 0]).all()
    return full


@pytest.mark.parametrize("k", range(len(R.CASES)), ids=IDS)
def test_geometry_on_the_devices_lists_equals_the_restatement(N, dev, k):
    c = R.CASES[k]
    K = R.KS[1 + k % 3]
    p = R.case_lists(c)[0]
    idx, _ = _knn(N, dev, _points(p, dev), K, want_d2=False)
    orient_to = (0.5, -3.0, 2.0) if k % 2 else None
    _check_geometry(N, dev, p, idx, 3, None if k % 3 else max(1, K // 2), orient_to, c.name)
    if K > 3:
        _check_geometry(N, dev, p, idx, 1, K, None if k % 2 else (0.0, 0.0, 0.0), c.name + "/k_s=1")


@pytest.mark.parametrize("name,K", [("sphere-4097", 16), ("nonfinite-900", 8), ("lattice-1728", 32), ("identical-200", 5), ("sphere-3", 2)])
def test_geometry_on_hand_made_lists_equals_the_restatement(N, dev, name, K):
    c = next(c for c in R.CASES if c.name == name)
    p = R.case_lists(c)[0]
    idx = R.handmade_lists(c.P, K, seed=K)
    _check_geometry(N, dev, p, idx, min(3, K), None, (1.0, 2.0, 3.0), name + "/handmade")
    _check_geometry(N, dev, p, idx, K, max(1, K - 1), None, name + "/handmade, no orientation")


@pytest.mark.parametrize("mode", ["isotropic", "surfel"])
def test_a_sphere_from_raw_points_to_images_and_three_adam_steps(N, dev, mode):
    from pcrender import camera, cloud, optim, raster_passes as rp
    c = next(c for c in R.CASES if c.name == "sphere-4097")
    p = R.case_lists(c)[0]
    pts = NC.to_device(p, dev)
    colors = (pts * 0.25 + 0.5).clamp(0, 1).contiguous()
    before = N.lib.gsr_d2h_count()
    g = cloud.gaussians_from_points(pts, colors, mode=mode, K=16, orient_to=(0.0, 0.0, 0.0))
    assert N.lib.gsr_d2h_count() == before
    assert sorted(g) == ["means3D", "normals", "opacities", "rotations", "scales", "shs"]
    assert all(v.dtype == torch.float32 and v.is_contiguous() and v.shape[0] == c.P and bool(torch.isfinite(v).all()) for v in g.values())
    # oriented away from the centre, the normals are the outward ones
    out_n = torch.nn.functional.normalize(pts, dim=1)
    assert float((g["normals"] * out_n).sum(1).min()) > 0
    assert float(torch.quantile(torch.rad2deg(torch.acos((g["normals"] * out_n).sum(1).clamp(-1, 1))), 0.99)) < R.NORMAL_P99_BAR_DEG
    sf, h, w = 4.0, 64, 64
    Hs = camera.circle_path(2, 0, 3, [90, 0])
    img = rp.render_passes(g["means3D"], g["opacities"], g["scales"], g["rotations"], g["shs"], Hs, h, w, 45.0, torch.zeros(3), sf,
                           normals=g["normals"], sh_degree=1, super_sample_rate=2)
    for k in ("rgb", "xyz_w", "hitmap", "normal"):
        assert img[k].shape == (1, 2, h, w, 3) and bool(torch.isfinite(img[k]).all()), k
    # inside the silhouette -- the unit sphere seen from 3 away under 45 degrees covers tan(asin(1/3)) / tan(22.5 deg) = 0.85 of the half
    # image; 0.75 of it is well inside -- the hit map has no hole
    yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    rr = torch.sqrt((yy - (h - 1) / 2.0) ** 2 + (xx - (w - 1) / 2.0) ** 2) / (h / 2.0)
    inside = rr < 0.75 * 0.85
    for v in range(2):
        hit = img["hitmap"][0, v, :, :, 0]
        assert float(hit[inside].min()) > 0.99, (mode, v, float(hit[inside].min()))
        # centre pixels: the normal pass against the analytic normal of the surface point the xyz pass shows
        centre = rr < 0.15
        n_img = torch.nn.functional.normalize(img["normal"][0, v][centre], dim=1)
        n_true = torch.nn.functional.normalize(img["xyz_w"][0, v][centre], dim=1)
        ang = torch.rad2deg(torch.acos((n_img * n_true).sum(1).abs().clamp(0, 1)))
        assert float(ang.max()) < R.NORMAL_P99_BAR_DEG, (mode, v, float(ang.max()))
    # three optimizer steps on the result, scales stored as logarithms
    gl = cloud.gaussians_from_points(pts, colors, mode=mode, K=16, log_scales=True, orient_to=(0.0, 0.0, 0.0))
    assert torch.allclose(gl["scales"].exp(), g["scales"], rtol=1e-5)
    names = ("means3D", "opacities", "scales", "rotations", "shs")
    params = {k: gl[k].clone().requires_grad_(True) for k in names}
    opt = optim.GaussianAdam(params, dict(means3D=1e-4, opacities=1e-2, scales=5e-3, rotations=1e-3, shs=2.5e-3))
    start = {k: v.detach().clone() for k, v in params.items()}
    for _ in range(3):
        out = rp.train_passes(params["means3D"], params["opacities"], params["scales"].exp(), params["rotations"], params["shs"], Hs, h, w,
                              45.0, torch.zeros(3), sf, normals=gl["normals"], sh_degree=1, super_sample_rate=2)
        loss = (out["rgb"] - 0.5).abs().mean() + (1 - out["hitmap"]).abs().mean()
        loss.backward()
        opt.step(zero_grads=True)
    assert opt.t == 3
    assert all(bool(torch.isfinite(v).all()) for v in params.values())
    assert any(not torch.equal(params[k].detach(), start[k]) for k in names)
