"""Float64 evaluation of the camera gradients of one view (test infrastructure): dL/d viewmatrix, projmatrix and campos from the
RENDER-level sums (dL/dmean2D, dL/dconic, dL/dcolour), the arbiter for gsr_backward_cameras.

Written from the formulas of include/gsr.h / DESIGN.md section 4e in the style and conventions of tests/fp64_backward.py: float32
inputs and constants promoted, focal length and clamp limits as the kernel computes them, the frustum clamp as the reference's
backward treats it (dL/dt_x = 0 where |t_x / t_z| was clamped, the clamped t_x a constant in dL/dt_z), the SH clamp mask of the
forward taken as given.  With m = (x, y, z, 1) the mean and r_k = (view[k], view[4+k], view[8+k]):

    conic    dL/dr0 += J00 dm0 + dt_x mean,  dL/dr1 += J11 dm1 + dt_y mean,  dL/dr2 += J02 dm0 + J12 dm1 + dt_z mean,
             dL/dview[12+k] += dt_k
    mean2D   dL/dproj[k + 4j] += gh_k m_j  (k = 0, 1, 3), gh0 = gx iw, gh1 = gy iw, gh3 = -(hx iw^2 gx + hy iw^2 gy)
    colour   dL/dcampos -= the view direction's share of dL/dmean
"""
import numpy as np

from fp64_backward import C1, C2, C3, F

LIVE_VIEW = [k + 4 * j for k in range(3) for j in range(4)]
LIVE_PROJ = [k + 4 * j for k in (0, 1, 3) for j in range(4)]
DEAD_VIEW, DEAD_PROJ = [3, 7, 11, 15], [2, 6, 10, 14]


def camera_backward_fp64(s, radii, clamped, dL_dmean2D, dL_dconic, dL_dcolor, dtype=np.float64):
    """s: oracle.Scene (one view); radii [P] int, clamped [P,3] bool (forward state); dL_dmean2D [P,>=2], dL_dconic [P,4] (x, y, -, w),
    dL_dcolor [P,3].  Returns dict(dL_dviewmatrix [16], dL_dprojmatrix [16], dL_dcampos [3]) in the flattening of the scene's own
    matrices.  dtype=np.float32 runs the same expressions (and the sum over the Gaussians) in single precision."""
    dt = dtype
    vis = np.asarray(radii) > 0
    idx = np.nonzero(vis)[0]
    n = idx.size
    p = s.means3D[idx].astype(dt)
    V = s.viewmatrix.astype(dt)
    Pm = s.projmatrix.astype(dt)
    g2 = np.asarray(dL_dmean2D, dt)[idx]
    gcon = np.asarray(dL_dconic, dt)[idx]
    gcol = np.asarray(dL_dcolor, dt)[idx]
    W3 = np.array([[V[0], V[4], V[8]], [V[1], V[5], V[9]], [V[2], V[6], V[10]]], dtype=dt)       # rows r0, r1, r2
    tr = np.array([V[12], V[13], V[14]], dtype=dt)
    fx = dt(F(s.W) / (F(2.0) * F(s.tanfovx)))
    fy = dt(F(s.H) / (F(2.0) * F(s.tanfovy)))
    limx, limy = dt(F(1.3) * F(s.tanfovx)), dt(F(1.3) * F(s.tanfovy))
    one = dt(1.0)
    dV, dP, dC = np.zeros(16, dt), np.zeros(16, dt), np.zeros(3, dt)
    if n == 0:
        return dict(dL_dviewmatrix=dV, dL_dprojmatrix=dP, dL_dcampos=dC)

    # ---- 3D covariance
    if s.cov3D_precomp is not None:
        c6 = s.cov3D_precomp[idx].astype(dt)
        S = np.zeros((n, 3, 3), dt)
        S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2] = c6.T
        S[:, 1, 0], S[:, 2, 0], S[:, 2, 1] = S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]
    else:
        q = s.rotations[idx].astype(dt)
        r, x, y, z = q.T
        R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                      np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                      np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
        sc = s.scales[idx].astype(dt) * dt(F(s.scale_modifier))
        S = np.einsum("nij,nj,nkj->nik", R, sc * sc, R)

    # ---- conic -> (a, b, c) -> rows of M -> Jacobian entries / view rows / view-space mean
    t = p @ W3.T + tr
    txtz, tytz = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    cx, cy = (txtz < -limx) | (txtz > limx), (tytz < -limy) | (tytz > limy)
    tx, ty, tz = np.clip(txtz, -limx, limx) * t[:, 2], np.clip(tytz, -limy, limy) * t[:, 2], t[:, 2]
    J00, J02, J11, J12 = fx / tz, -fx * tx / (tz * tz), fy / tz, -fy * ty / (tz * tz)
    m0 = J00[:, None] * W3[0] + J02[:, None] * W3[2]
    m1 = J11[:, None] * W3[1] + J12[:, None] * W3[2]
    u, w = np.einsum("nij,nj->ni", S, m0), np.einsum("nij,nj->ni", S, m1)
    a = np.einsum("ni,ni->n", m0, u) + dt(F(0.3))
    b = np.einsum("ni,ni->n", m0, w)
    c = np.einsum("ni,ni->n", m1, w) + dt(F(0.3))
    gA, gB, gC = gcon[:, 0], gcon[:, 1], gcon[:, 3]
    det = a * c - b * b
    Dn = one / (det * det + dt(F(0.0000001)))
    da = Dn * (-c * c * gA + 2 * b * c * gB + (det - a * c) * gC)
    dc = Dn * (-a * a * gC + 2 * a * b * gB + (det - a * c) * gA)
    db = Dn * 2 * (b * c * gA - (det + 2 * b * b) * gB + a * b * gC)
    dm0 = 2 * da[:, None] * u + db[:, None] * w
    dm1 = 2 * dc[:, None] * w + db[:, None] * u
    dJ00, dJ02, dJ11, dJ12 = dm0 @ W3[0], dm0 @ W3[2], dm1 @ W3[1], dm1 @ W3[2]
    iz = one / tz
    dtx = np.where(cx, dt(0.0), -fx * iz * iz * dJ02)
    dty = np.where(cy, dt(0.0), -fy * iz * iz * dJ12)
    dtz = -(fx * dJ00 + fy * dJ11) * iz * iz + 2 * (fx * tx * dJ02 + fy * ty * dJ12) * iz ** 3
    dr = [J00[:, None] * dm0 + dtx[:, None] * p,
          J11[:, None] * dm1 + dty[:, None] * p,
          J02[:, None] * dm0 + J12[:, None] * dm1 + dtz[:, None] * p]
    for k in range(3):
        for j in range(3):
            dV[k + 4 * j] = dr[k][:, j].sum(dtype=dt)
    dV[12], dV[13], dV[14] = dtx.sum(dtype=dt), dty.sum(dtype=dt), dtz.sum(dtype=dt)

    # ---- mean2D -> the rows of proj the perspective divide reads
    hom = lambda row: Pm[row] * p[:, 0] + Pm[4 + row] * p[:, 1] + Pm[8 + row] * p[:, 2] + Pm[12 + row]   # noqa: E731
    hx, hy, hw = hom(0), hom(1), hom(3)
    iw = one / (hw + dt(F(0.0000001)))
    kx, ky = hx * iw * iw, hy * iw * iw
    gh = {0: g2[:, 0] * iw, 1: g2[:, 1] * iw, 3: -(kx * g2[:, 0] + ky * g2[:, 1])}
    m4 = np.concatenate([p, np.ones((n, 1), dt)], 1)
    for k in (0, 1, 3):
        for j in range(4):
            dP[k + 4 * j] = (gh[k] * m4[:, j]).sum(dtype=dt)

    # ---- colour -> view direction -> campos
    if s.shs is not None and s.sh_degree > 0:
        sh = s.shs[idx].astype(dt)
        D = s.sh_degree
        do = p - s.campos.astype(dt)
        ln = np.linalg.norm(do, axis=1, keepdims=True).astype(dt)
        d = do / ln
        x, y, z = d.T
        gr = gcol * (~np.asarray(clamped, bool)[idx])
        zero = np.zeros(n, dt)
        c1, c2, c3 = dt(C1), [dt(v) for v in C2], [dt(v) for v in C3]
        ddx = [zero, zero, zero, zero - c1]
        ddy = [zero, zero - c1, zero, zero]
        ddz = [zero, zero, zero + c1, zero]
        if D > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            ddx += [c2[0] * y, zero, c2[2] * (-2 * x), c2[3] * z, c2[4] * 2 * x]
            ddy += [c2[0] * x, c2[1] * z, c2[2] * (-2 * y), zero, c2[4] * (-2 * y)]
            ddz += [zero, c2[1] * y, c2[2] * 4 * z, c2[3] * x, zero]
        if D > 2:
            ddx += [c3[0] * 6 * xy, c3[1] * yz, c3[2] * (-2) * xy, c3[3] * (-6) * xz, c3[4] * (-3 * xx + 4 * zz - yy), c3[5] * 2 * xz,
                    c3[6] * 3 * (xx - yy)]
            ddy += [c3[0] * 3 * (xx - yy), c3[1] * xz, c3[2] * (-3 * yy + 4 * zz - xx), c3[3] * (-6) * yz, c3[4] * (-2) * xy,
                    c3[5] * (-2) * yz, c3[6] * (-6) * xy]
            ddz += [zero, c3[1] * xy, c3[2] * 8 * yz, c3[3] * 3 * (2 * zz - xx - yy), c3[4] * 8 * xz, c3[5] * (xx - yy), zero]
        K = len(ddx)
        dRx = sum(ddx[k][:, None] * sh[:, k, :] for k in range(K))
        dRy = sum(ddy[k][:, None] * sh[:, k, :] for k in range(K))
        dRz = sum(ddz[k][:, None] * sh[:, k, :] for k in range(K))
        ddir = np.stack([(dRx * gr).sum(1), (dRy * gr).sum(1), (dRz * gr).sum(1)], -1)
        share = (ddir - d * (d * ddir).sum(1, keepdims=True)) / ln          # what the mean gets through the view direction
        dC = -share.sum(0, dtype=dt)
    return dict(dL_dviewmatrix=dV.astype(dt), dL_dprojmatrix=dP.astype(dt), dL_dcampos=np.asarray(dC, dt))
