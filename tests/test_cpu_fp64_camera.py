"""The float64 arbiter of the camera gradients (tests/fp64_camera.py) held to (1) central differences of a float64 numpy forward of the
per-Gaussian map (view, proj, campos) -> (ndc mean2D, conic, SH colour) and (2) the translation identity that ties it to
tests/fp64_backward.py, the module the existing gradients are already held to."""
import numpy as np
import pytest

import util
from fp64_backward import C0, C1, C2, C3, gaussian_backward_fp64
from fp64_camera import DEAD_PROJ, DEAD_VIEW, LIVE_PROJ, LIVE_VIEW, camera_backward_fp64
from camera_cases import census, cloud, mixed_scene, pose, translation_identity


def _sh_basis(d, D):
    x, y, z = d.T
    b = [np.full(x.shape, C0)]
    if D > 0:
        b += [-C1 * y, C1 * z, -C1 * x]
    if D > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if D > 2:
        b += [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
              C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
    return np.stack(b, 1)                                                   # [n, K]


def forward_fp64(s, V, Pm, campos):
    """The per-Gaussian forward map in float64: (ndc mean2D [P,2], conic (A, B, C) [P,3], colour before the clamp [P,3]) for view /
    proj [16] and campos [3] given as float64 (the scene's other inputs promoted).  No frustum clamp: for clouds inside it."""
    p = s.means3D.astype(np.float64)
    W3 = np.array([[V[0], V[4], V[8]], [V[1], V[5], V[9]], [V[2], V[6], V[10]]])
    t = p @ W3.T + np.array([V[12], V[13], V[14]])
    fx = np.float64(np.float32(s.W) / (np.float32(2.0) * np.float32(s.tanfovx)))
    fy = np.float64(np.float32(s.H) / (np.float32(2.0) * np.float32(s.tanfovy)))
    tx, ty, tz = t.T
    m0 = (fx / tz)[:, None] * W3[0] + (-fx * tx / (tz * tz))[:, None] * W3[2]
    m1 = (fy / tz)[:, None] * W3[1] + (-fy * ty / (tz * tz))[:, None] * W3[2]
    q = s.rotations.astype(np.float64)
    r, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    sc = s.scales.astype(np.float64) * np.float64(np.float32(s.scale_modifier))
    S = np.einsum("nij,nj,nkj->nik", R, sc * sc, R)
    u, w = np.einsum("nij,nj->ni", S, m0), np.einsum("nij,nj->ni", S, m1)
    a = np.einsum("ni,ni->n", m0, u) + np.float64(np.float32(0.3))
    b = np.einsum("ni,ni->n", m0, w)
    c = np.einsum("ni,ni->n", m1, w) + np.float64(np.float32(0.3))
    det = a * c - b * b
    conic = np.stack([c / det, -b / det, a / det], 1)
    hom = lambda row: Pm[row] * p[:, 0] + Pm[4 + row] * p[:, 1] + Pm[8 + row] * p[:, 2] + Pm[12 + row]   # noqa: E731
    iw = 1.0 / (hom(3) + np.float64(np.float32(0.0000001)))
    ndc = np.stack([hom(0) * iw, hom(1) * iw], 1)
    do = p - campos
    d = do / np.linalg.norm(do, axis=1, keepdims=True)
    K = (s.sh_degree + 1) ** 2
    rgb = np.einsum("nk,nkc->nc", _sh_basis(d, s.sh_degree), s.shs[:, :K, :].astype(np.float64)) + 0.5
    return ndc, conic, rgb, det


@pytest.mark.parametrize("degree", [3, 0])
def test_arbiter_matches_central_differences(degree):
    W = H = 64
    g = cloud(40, 100 + degree, degree)
    s = util.scene_from(g, util._view_arrays(pose(7), W, H, 60.0), W, H)
    V0, P0, C0_ = s.viewmatrix.astype(np.float64), s.projmatrix.astype(np.float64), s.campos.astype(np.float64)
    ndc, conic, rgb, det = forward_fp64(s, V0, P0, C0_)
    # inside the 1.3 tanfov clamp, footprints of a few pixels (1 / (det^2 + 1e-7) is then 1 / det^2 to 1e-9), no colour at its clamp
    t = s.means3D.astype(np.float64) @ np.array([[V0[0], V0[4], V0[8]], [V0[1], V0[5], V0[9]], [V0[2], V0[6], V0[10]]]).T + V0[12:15]
    assert (np.abs(t[:, 0] / t[:, 2]) < 1.3 * s.tanfovx).all() and (np.abs(t[:, 1] / t[:, 2]) < 1.3 * s.tanfovy).all() and (t[:, 2] > 0.2).all()
    assert det.min() > 10.0
    assert np.abs(rgb).min() > 1e-3
    clamped = rgb < 0
    if degree:
        assert clamped.any() and not clamped.all()
    rng = np.random.default_rng(5)
    c_ndc, c_con, c_rgb = rng.standard_normal((s.P, 2)), rng.standard_normal((s.P, 3)), rng.standard_normal((s.P, 3))

    def loss(V, Pm, Cm):
        n_, k_, r_, _ = forward_fp64(s, V, Pm, Cm)
        return (c_ndc * n_).sum() + (c_con * k_).sum() + (c_rgb * np.maximum(r_, 0.0)).sum()

    # the records hold HALF of dL/d conic.y (the render backward's convention, which the factor 2 of dL/db undoes)
    dcon = np.stack([c_con[:, 0], 0.5 * c_con[:, 1], np.zeros(s.P), c_con[:, 2]], 1)
    got = camera_backward_fp64(s, np.ones(s.P, np.int32), clamped, np.concatenate([c_ndc, np.zeros((s.P, 1))], 1), dcon, c_rgb)
    h = 1e-5
    base = (V0, P0, C0_)
    for which, name, live, dead in ((0, "dL_dviewmatrix", LIVE_VIEW, DEAD_VIEW), (1, "dL_dprojmatrix", LIVE_PROJ, DEAD_PROJ),
                                    (2, "dL_dcampos", [0, 1, 2], [])):
        fd = np.zeros_like(base[which])
        for e in live:
            args_p, args_m = [x.copy() for x in base], [x.copy() for x in base]
            args_p[which][e] += h
            args_m[which][e] -= h
            fd[e] = (loss(*args_p) - loss(*args_m)) / (2 * h)
        scale = max(np.abs(fd).max(), np.abs(got[name]).max())
        if name == "dL_dcampos" and degree == 0:
            assert (got[name] == 0).all() and np.abs(fd).max() <= 1e-9
            continue
        assert scale > 0
        err = np.abs(got[name] - fd)[live].max()
        print("degree %d %s: max|arbiter - central difference| = %.3g of max|g| = %.3g" % (degree, name, err, scale))
        assert err <= 1e-6 * scale, (name, err, scale)
        assert (got[name][dead] == 0).all(), name


def test_translation_identity_ties_the_arbiter_to_the_cloud_chain():
    from oracle.oracle import Oracle
    s = mixed_scene()
    fwd = Oracle().forward(s)
    out, behind, col = census(s, fwd)
    assert out.size and behind.size and col.size, (out.size, behind.size, col.size)
    rng = np.random.default_rng(9)
    g2 = np.concatenate([rng.standard_normal((s.P, 2)), np.zeros((s.P, 1))], 1)
    gcon = rng.standard_normal((s.P, 4))
    gcol = rng.standard_normal((s.P, 3))
    with np.errstate(all="ignore"):
        gm = gaussian_backward_fp64(s, fwd["radii"], fwd["clamped"], g2, gcon, gcol)["dL_dmean3D"]
    cg = camera_backward_fp64(s, fwd["radii"], fwd["clamped"], g2, gcon, gcol)
    left, right = translation_identity([s], gm, [cg])
    bound = 1e-12 * np.abs(gm).sum(0)
    print("translation identity: |left - right| =", np.abs(left - right), "bound", bound)
    assert (np.abs(left - right) <= bound).all(), (left, right)
    assert (cg["dL_dviewmatrix"][DEAD_VIEW] == 0).all() and (cg["dL_dprojmatrix"][DEAD_PROJ] == 0).all()
