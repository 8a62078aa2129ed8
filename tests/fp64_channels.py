"""Float64 reference for the extra render channels (test infrastructure, like tests/fp64_backward.py).

A channels render composites NX per-Gaussian values e_k = extra_k * view_scale_k with the colour's alphas:
    image_k(p) = sum_i e_ik alpha_i(p) T_i(p) + T_final(p) bg_extra_k
so  dL/d extra[i][k] = view_scale_k * sum_p alpha_i(p) T_i(p) dL_dextra_k(p).

extra_render_fp64 evaluates both from the oracle's forward state of one view, written from these formulas: which entries a
pixel takes (the power > 0 skip, the 1/255 cut, the 0.99 clamp, the T < 1e-4 stop) is decided in float32 with the oracle's
expression order, alpha and T of the taken entries and every sum are float64 (as orc_render_backward_fp64 takes them).

channels_backward_fp64 builds the render-level sums a channels backward must reproduce: the float64 render backward of the
colour run plus one colors_precomp run per group of three channels (the extras share the alphas, so their share of the
mean2D / conic / opacity sums is exactly such a run's), and the per-Gaussian chain of tests/fp64_backward.py on those sums.
"""
import numpy as np

import util
from fp64_backward import gaussian_backward_fp64

F = np.float32


def _tile_walk(fwd, t):
    """(ids, pixel indices, float64 weights alpha T [L, n], float32 stop decisions replayed) for tile t of a forward dict"""
    W, H = fwd["W"], fwd["H"]
    gx = (W + 15) // 16
    r0, r1 = (int(v) for v in fwd["ranges"][t])
    ty, tx = divmod(t, gx)
    ys, xs = np.meshgrid(np.arange(ty * 16, min(ty * 16 + 16, H)), np.arange(tx * 16, min(tx * 16 + 16, W)), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    pix = ys * W + xs
    n = pix.size
    if r1 <= r0:
        return None, pix, None, np.zeros(n, np.int64), np.ones(n, np.float32), np.ones(n)
    ids = fwd["vals"][r0:r1].astype(np.int64)
    m2 = fwd["means2D"].astype(F)
    co = fwd["conic_opacity"].astype(F)
    A, B, C, O = (co[ids, k][:, None] for k in range(4))
    mx, my = m2[ids, 0][:, None], m2[ids, 1][:, None]
    # float32 decisions, one rounding per operation (gsr_oracle.c is built with -ffp-contract=off)
    dx, dy = mx - xs.astype(F)[None, :], my - ys.astype(F)[None, :]
    power = F(-0.5) * (A * dx * dx + C * dy * dy) - B * dx * dy
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a32 = np.minimum(F(0.99), O * np.exp(power.astype(np.float64)).astype(F))
    hit = ~(power > 0) & ~(a32 < F(1.0) / F(255.0))
    # the float32 transmittance chain: skipped entries multiply by 1 (exact); the first taken entry whose T (1 - alpha) falls
    # below 1e-4 stops the pixel and is not taken
    f32 = np.where(hit, F(1.0) - a32, F(1.0)).astype(F)
    after = np.multiply.accumulate(f32, axis=0, dtype=F)
    stop = hit & (after < F(0.0001))
    L = ids.size
    first_stop = np.where(stop.any(0), stop.argmax(0), L)
    taken = hit & (np.arange(L)[:, None] < first_stop[None, :])
    last = np.where(taken.any(0), L - taken[::-1].argmax(0), 0)
    T32 = np.where(last > 0, after[np.maximum(last - 1, 0), np.arange(n)], F(1.0)).astype(F)
    # float64 alpha and transmittance of the taken entries
    ddx = m2[ids, 0][:, None].astype(np.float64) - xs[None, :]
    ddy = m2[ids, 1][:, None].astype(np.float64) - ys[None, :]
    pw = -0.5 * (A * ddx * ddx + C * ddy * ddy) - B.astype(np.float64) * ddx * ddy
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a64 = np.minimum(O.astype(np.float64) * np.exp(pw), np.float64(F(0.99)))
    a64 = np.where(taken, a64, 0.0)
    fac = 1.0 - a64
    T_after = np.cumprod(fac, axis=0)
    T_before = np.concatenate([np.ones((1, n)), T_after[:-1]], 0)
    return ids, pix, a64 * T_before, last, T32, T_after[-1]


def extra_render_fp64(fwd, values, bg_extra, dL_dextra=None, scale=None):
    """fwd: Oracle.forward dict of one view; values [P, nx] (this view's, unscaled), bg_extra [nx], dL_dextra [nx, H, W] or None,
    scale [nx] or None (= 1).  Returns dict(image [nx, H, W], grad [P, nx] (scale_k sum_p alpha T dL_dextra_k; None without
    dL_dextra), final_T [H, W]) in float64.  Asserts that the replayed decisions give the oracle's n_contrib and final_T."""
    W, H = fwd["W"], fwd["H"]
    nx = np.asarray(values).shape[-1]
    P = np.asarray(values).shape[0]
    sc = np.ones(nx) if scale is None else np.asarray(scale, np.float64).reshape(nx)
    # the values as the forward composites them: the float32 product values x scale (float64 values: the exact product)
    vals = np.asarray(values)
    vals = vals if vals.dtype == np.float64 else vals.astype(F)
    e = (vals * sc.astype(vals.dtype)[None, :]).astype(np.float64)
    img = np.zeros((nx, H * W))
    Tf = np.ones(H * W)
    grad = None if dL_dextra is None else np.zeros((P, nx))
    dlx = None if dL_dextra is None else np.asarray(dL_dextra, np.float64).reshape(nx, H * W)
    if P and fwd["R"]:
        nc = np.zeros(H * W, np.int64)
        t32 = np.ones(H * W, np.float32)
        T = fwd["ranges"].shape[0]
        for t in range(T):
            ids, pix, w, last, T32, Tend = _tile_walk(fwd, t)
            nc[pix], t32[pix], Tf[pix] = last, T32, Tend
            if ids is None:
                continue
            img[:, pix] += (w.T @ e[ids]).T
            if grad is not None:
                grad[ids] += (w @ dlx[:, pix].T) * sc[None, :]   # (one pair per (tile, Gaussian): ids are unique here)
        assert np.array_equal(nc, fwd["n_contrib"].reshape(-1).astype(np.int64)), \
            "replayed float32 decisions differ from the oracle's n_contrib at %d pixels" % int((nc != fwd["n_contrib"].reshape(-1)).sum())
        # (numpy's exp rounded to float32 and glibc's expf differ in the last bit now and then: a few ulp of T, no decision)
        u = util.ulp_diff(t32, fwd["final_T"].reshape(-1)).max()
        assert u <= 32, "replayed float32 transmittance differs from final_T by %d ulp" % u
    img += Tf[None, :] * np.asarray(bg_extra, F).astype(np.float64)[:, None]
    return dict(image=img.reshape(nx, H, W), grad=grad, final_T=Tf.reshape(H, W))


def _groups(nx):
    return [list(range(k0, min(k0 + 3, nx))) for k0 in range(0, nx, 3)]


def with_colours(s, cols, bg):
    """the Scene s with colors_precomp = cols (no SH) and background bg: what one group of three extra channels renders like"""
    kw = dict(W=s.W, H=s.H, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=bg, means3D=s.means3D, opacities=s.opacities,
              viewmatrix=s.viewmatrix, projmatrix=s.projmatrix, campos=s.campos, colors_precomp=cols, scales=s.scales,
              rotations=s.rotations, cov3D_precomp=s.cov3D_precomp, scale_modifier=s.scale_modifier, prefiltered=s.prefiltered)
    return util.Scene(**kw)


def channels_backward_fp64(oracle, g, views, W, H, dense_extra, scale, bg_extra, dL_dpix, dL_dextra, bg=(0.0, 0.0, 0.0),
                           mode="sh", use_cov3d=False, nthreads=16):
    """The render-level sums of a channels backward, per view, and its per-Gaussian gradients summed over the views, in float64.
    g: the cloud (util.scene_from's dict; colors_precomp for mode="colors"); views: camera dicts; dense_extra [V, P, nx] (each view's
    values, unscaled); scale [V, nx] or None; bg_extra [nx]; dL_dpix [V, 3, H, W]; dL_dextra [V, nx, H, W].  See channels_backward_fp64_scenes."""
    scenes = [util.scene_from(g, v, W, H, bg=bg, mode=mode, use_cov3d=use_cov3d) for v in views]
    return channels_backward_fp64_scenes(oracle, scenes, dense_extra, scale, bg_extra, dL_dpix, dL_dextra, nthreads=nthreads)


def channels_backward_fp64_scenes(oracle, scenes, dense_extra, scale, bg_extra, dL_dpix, dL_dextra, nthreads=16):
    """channels_backward_fp64 with one oracle Scene per view (the colour run: cloud, camera, colours, background).
    Returns dict(views=[dict(mean2D [P,2], conic [P,3] (x, y, w), opacity [P], colour [P,3], extra [P, nx], fwd, scene,
                             exact / f32 = the render-level sums as grad_ladder.Float64.views() names them: dL_dmean2D [P,3],
                             dL_dconic [P,4], dL_dcolor [P,3], in float64 / as the double sums of the oracle's float32 terms)],
                 grads=dict(dL_dmean2D [P,3], dL_dcolor, dL_dopacity [P,1], dL_dmean3D, dL_dcov3D, dL_dsh?, dL_dscale?, dL_drot?))."""
    dense = np.asarray(dense_extra, F)
    V, P, nx = dense.shape
    sc = np.ones((V, nx), F) if scale is None else np.asarray(scale, F).reshape(V, nx)
    out, tot = [], {}

    def add(k, a):
        tot[k] = tot.get(k, 0.0) + np.asarray(a, np.float64)

    for v, s in enumerate(scenes):
        H, W = s.H, s.W
        fwd, gr = oracle.forward_backward(s, np.asarray(dL_dpix[v], F), exact=True, nthreads=nthreads)
        if P:
            ex = gr["exact"]
            m2, con, op = ex["dL_dmean2D"][:, :2].copy(), ex["dL_dconic"][:, [0, 1, 3]].copy(), ex["dL_dopacity"][:, 0].copy()
            col = ex["dL_dcolor"].copy()
            # the double sums of the oracle's float32 terms of the same runs (the noise model of tests/grad_ladder.py)
            m2_32, con_32 = gr["dL_dmean2D"].astype(np.float64), gr["dL_dconic"].astype(np.float64)
        else:
            m2, con, op, col = np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3))
            m2_32, con_32 = np.zeros((0, 3)), np.zeros((0, 4))
        gx = np.zeros((P, nx))
        for ks in _groups(nx):
            cols = np.zeros((P, 3), F)
            cols[:, :len(ks)] = dense[v][:, ks] * sc[v, ks]
            b3 = np.zeros(3, F)
            b3[:len(ks)] = np.asarray(bg_extra, F)[ks]
            dl = np.zeros((3, H, W), F)
            dl[:len(ks)] = np.asarray(dL_dextra[v], F)[ks]
            if not P:
                continue
            _, gxr = oracle.forward_backward(with_colours(s, cols, b3), dl, exact=True, nthreads=nthreads)
            e = gxr["exact"]
            m2 += e["dL_dmean2D"][:, :2]
            con += e["dL_dconic"][:, [0, 1, 3]]
            op += e["dL_dopacity"][:, 0]
            gx[:, ks] = e["dL_dcolor"][:, :len(ks)] * sc[v, ks].astype(np.float64)
            m2_32 = m2_32 + gxr["dL_dmean2D"]
            con_32 = con_32 + gxr["dL_dconic"]
        conic4 = np.zeros((P, 4))
        conic4[:, [0, 1, 3]] = con
        if P:
            chain = gaussian_backward_fp64(s, fwd["radii"], fwd["clamped"], np.concatenate([m2, np.zeros((P, 1))], 1), conic4, col)
            for k, a in chain.items():
                add(k, a)
        add("dL_dmean2D", np.concatenate([m2, np.zeros((P, 1))], 1))
        add("dL_dcolor", col)
        add("dL_dopacity", op[:, None])
        out.append(dict(mean2D=m2, conic=con, opacity=op, colour=col, extra=gx, fwd=fwd, scene=s,
                        exact=dict(dL_dmean2D=np.concatenate([m2, np.zeros((P, 1))], 1), dL_dconic=conic4, dL_dcolor=col),
                        f32=dict(dL_dmean2D=m2_32, dL_dconic=con_32,
                                 dL_dcolor=gr["dL_dcolor"].astype(np.float64) if P else np.zeros((0, 3)))))
    return dict(views=out, grads=tot)


def fold_extra(gx, layout):
    """per-view dL/d values [V, P, nx] -> the layout of the values: 0 shared [P, nx], 1 per view [V, P, nx], 2 split (([P,4], [V,P,4]))"""
    gx = np.asarray(gx, np.float64)
    if layout == 0:
        return gx.sum(0)
    if layout == 1:
        return gx
    return gx[:, :, :4].sum(0), gx[:, :, 4:]
