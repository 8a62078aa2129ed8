"""One scene family for the row spans of the footprint clipping (csrc/tile_cull.hpp clip_rect_to_footprint, read back by binning.hip
k_duplicate): thin splats rotated about the view axis, each with its opacity set so that the best pixel of one tile DIAGONAL to its
centre tile sits within a hair of the alpha = 1/255 cut -- the tiles a row span decides about.  Importable without a GPU: numpy,
util, the CPU oracle.

  case(variant, oracle)   the scene (identity camera, 667 x 599: 42 x 38 tiles, the last column and row partial), a second view of
                          the same cloud, and per splat the targeted tile and the delta it was placed at; built once per variant
  census(fwd, c)          from a forward's float32 means2D / conic_opacity (the oracle's here, the reference build's on the GPU):
                          how close to the cut the targets came, the grazing pixels, and the clipped boxes' sizes in tiles

About 1 500 splats: long sigma 6-25 pixels, axis ratio 4-20, angles 20-70 degrees and their mirrors; a sixth with their means in
the border tiles or up to 30 pixels off a side of the image; a tenth sized (longer, at the steep and the flat end of the angles) so
that the clipped box comes out 8 or 9 tile rows high or 15 or 16 columns wide, the limits of the span encoding.  Variants: 0 as
described, 1 the covariances handed over precomputed, 2 axis ratios 10-20 only."""
import math

import numpy as np

import util

F = np.float32
W, H = 667, 599
GX, GY = (W + 15) // 16, (H + 15) // 16
Z0 = 2.0
FOV = 60.0
P = 1500
REACH = 7                 # candidate tiles: up to this many tiles from the centre tile in x and in y
POWER_RANGE = (-5.3, -0.5)
VARIANTS = [0, 1, 2]
_CASES = {}


def _cloud(variant):
    rng = np.random.default_rng(31 + variant)
    view = util.identity_camera(W, H, FOV)
    fx, fy = W / (2.0 * view["tanfovx"]), H / (2.0 * view["tanfovy"])
    i = np.arange(P)
    sized = i % 10 == 3
    border = (i % 6 == 0) & ~sized
    tall = sized & (i % 20 == 3)                       # 8 / 9 rows; the other sized ones: 15 / 16 columns
    long_px = rng.uniform(6.0, 25.0, P)
    ratio = np.exp(rng.uniform(math.log(10.0 if variant == 2 else 4.0), math.log(20.0), P))
    ang = np.radians(rng.uniform(20.0, 70.0, P))
    # sized: at tau = log(255 o) = 4 the box reaches 2.83 sigma sin / cos(angle) from the mean: about 60 pixels up and down make 8 or 9
    # rows, about 118 left and right 15 or 16 columns (and then few enough rows for the encoding: a flat angle)
    ang = np.where(tall, np.radians(rng.uniform(55.0, 70.0, P)), np.where(sized, np.radians(rng.uniform(20.0, 23.0, P)), ang))
    long_px = np.where(tall, rng.uniform(56.0, 66.0, P) / (2.83 * np.sin(ang)), np.where(sized, rng.uniform(112.0, 124.0, P) / (2.83 * np.cos(ang)), long_px))
    ang = np.where(rng.random(P) < 0.5, ang, math.pi - ang)
    px, py = rng.uniform(40.0, W - 40.0, P), rng.uniform(40.0, H - 40.0, P)
    px = np.where(sized, rng.uniform(150.0, W - 150.0, P), px)
    py = np.where(sized, rng.uniform(110.0, H - 110.0, P), py)
    # border: one coordinate in the first or the last tile or up to 30 pixels outside, the other anywhere from 30 pixels outside
    side = rng.integers(0, 4, P)
    near = rng.uniform(-30.0, 16.0, P)
    bx = np.where(side == 0, near, np.where(side == 1, W - 1 - near, rng.uniform(-30.0, W + 30.0, P)))
    by = np.where(side == 2, near, np.where(side == 3, H - 1 - near, rng.uniform(-30.0, H + 30.0, P)))
    px, py = np.where(border, bx, px), np.where(border, by, py)
    # pixel -> world at depth Z0: ndc2Pix of the projected point is affine in x / z at the identity camera
    pm = np.asarray(view["projmatrix"], np.float64).reshape(4, 4)
    means = np.stack([(px - (W - 1) / 2.0) / (0.5 * W * pm[0, 0]) * Z0, (py - (H - 1) / 2.0) / (0.5 * H * pm[1, 1]) * Z0, np.full(P, Z0)], 1)
    scales = np.stack([long_px * Z0 / fx, long_px / ratio * Z0 / fy, long_px / ratio * Z0 / fx], 1)
    rots = np.stack([np.cos(ang / 2), np.zeros(P), np.zeros(P), np.sin(ang / 2)], 1)
    g = dict(means3D=means.astype(F), scales=scales.astype(F), rotations=rots.astype(F), opacities=np.full((P, 1), 0.3, F),
             shs=(0.4 * rng.standard_normal((P, 4, 3))).astype(F), sh_degree=1)
    return g, view, dict(sized=sized, border=border, tall=tall), rng


def _second_view():
    """the identity camera moved a little sideways and up: other fractions of a pixel, other spans"""
    c2w = np.eye(4, dtype=F)
    c2w[:3, 3] = (0.013, -0.007, 0.0)
    return util._view_arrays(c2w, W, H, FOV)


def tile_best_powers(m2, co, i):
    """The largest float32 power (the kernels' expression, one rounding per operation) over the pixel centres inside the image of
    every tile within REACH of splat i's centre tile: (first tile x, first tile y, best [2 REACH + 1, 2 REACH + 1] with -inf for
    tiles outside the image, the pixel (x, y) it is reached at [.., .., 2])."""
    n = 2 * REACH + 1
    tx0, ty0 = int(math.floor(m2[i, 0] / 16.0)) - REACH, int(math.floor(m2[i, 1] / 16.0)) - REACH
    xs = (np.arange(16 * n) + 16 * tx0)
    ys = (np.arange(16 * n) + 16 * ty0)
    A, B, C = (F(co[i, k]) for k in range(3))
    dx = (F(m2[i, 0]) - xs.astype(F))[None, :]
    dy = (F(m2[i, 1]) - ys.astype(F))[:, None]
    power = F(-0.5) * (A * dx * dx + C * dy * dy) - B * dx * dy
    assert power.dtype == F
    ok = ((xs >= 0) & (xs < W))[None, :] & ((ys >= 0) & (ys < H))[:, None]
    power = np.where(ok, power, -np.inf).reshape(n, 16, n, 16).transpose(0, 2, 1, 3).reshape(n, n, 256)
    at = power.argmax(2)
    best = np.take_along_axis(power, at[:, :, None], 2)[:, :, 0]
    tyy, txx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pix = np.stack([16 * (tx0 + txx) + at % 16, 16 * (ty0 + tyy) + at // 16], 2)
    return tx0, ty0, best, pix


def box_tiles(m2, co, o):
    """(columns, rows) of the clipped box of every splat, in tiles inside the image: the bounding box of d^T conic d <= 2 log(255 o)
    around the mean, in float64 -- the clip's own box without its rounding allowances (a few 1e-4 of its half widths)"""
    A, B, C = (co[:, k].astype(np.float64) for k in range(3))
    det = A * C - B * B
    with np.errstate(invalid="ignore", divide="ignore"):
        k = 2.0 * np.log(255.0 * np.asarray(o, np.float64))
        hx, hy = np.sqrt(k * C / det), np.sqrt(k * A / det)
    x, y = m2[:, 0].astype(np.float64), m2[:, 1].astype(np.float64)
    ok = np.isfinite(hx) & np.isfinite(hy)
    hx, hy = np.where(ok, hx, 0.0), np.where(ok, hy, 0.0)
    c0, c1 = np.clip(np.floor(np.ceil(x - hx) / 16.0), 0, GX), np.clip(np.floor(np.floor(x + hx) / 16.0) + 1, 0, GX)
    r0, r1 = np.clip(np.floor(np.ceil(y - hy) / 16.0), 0, GY), np.clip(np.floor(np.floor(y + hy) / 16.0) + 1, 0, GY)
    return np.where(ok, np.maximum(c1 - c0, 0), 0).astype(int), np.where(ok, np.maximum(r1 - r0, 0), 0).astype(int)


def case(variant, oracle):
    if variant in _CASES:
        return _CASES[variant]
    g, view, kinds, rng = _cloud(variant)
    use_cov3d = variant == 1
    s0 = util.scene_from(g, view, W, H, bg=(0.1, 0.2, 0.3), use_cov3d=use_cov3d)
    o = oracle.forward(s0)
    m2, co = o["means2D"].astype(F), o["conic_opacity"].astype(F)
    vis = o["radii"] > 0
    # the relative offsets of the targeted power from the cut: dense within +-3e-4, a few further out
    deltas = np.concatenate([np.linspace(-3e-4, 3e-4, P - 8), [-3e-3, -1e-3, 1e-3, 3e-3, -2e-2, 2e-2, -1e-6, 1e-6]])[rng.permutation(P)]
    target = np.full((P, 2), -1, int)
    pixel = np.full((P, 2), -1, int)
    best = np.zeros(P, F)
    opac = g["opacities"].copy()
    off = np.arange(-REACH, REACH + 1)
    diagonal = (off[:, None] != 0) & (off[None, :] != 0)
    for i in np.nonzero(vis)[0]:
        tx0, ty0, b, pix = tile_best_powers(m2, co, i)
        cand = np.argwhere(diagonal & (b >= POWER_RANGE[0]) & (b <= POWER_RANGE[1]))
        if cand.size == 0:
            continue
        pick = cand[rng.integers(0, len(cand))]
        if kinds["sized"][i]:
            # the target decides the opacity and the opacity the box: a target that brings the box to the encoding's limits, if any
            oo = np.exp(-b[cand[:, 0], cand[:, 1]].astype(np.float64)) / 255.0
            cols, rows = box_tiles(np.repeat(m2[i:i + 1], len(cand), 0), np.repeat(co[i:i + 1], len(cand), 0), oo)
            hit = np.nonzero(np.isin(rows, (8, 9)) if kinds["tall"][i] else (np.isin(cols, (15, 16)) & (rows <= 8)))[0]
            if hit.size:
                pick = cand[hit[rng.integers(0, hit.size)]]
        best[i] = b[pick[0], pick[1]]
        target[i] = (tx0 + pick[1], ty0 + pick[0])
        pixel[i] = pix[pick[0], pick[1]]
        # power = thr (1 + delta) with thr = -log(255 o)
        opac[i, 0] = F(math.exp(-float(best[i]) / (1.0 + deltas[i])) / 255.0)
    g = dict(g, opacities=opac)
    scene = util.scene_from(g, view, W, H, bg=(0.1, 0.2, 0.3), use_cov3d=use_cov3d)
    scene2 = util.scene_from(g, _second_view(), W, H, bg=(0.1, 0.2, 0.3), use_cov3d=use_cov3d)
    c = dict(variant=variant, g=g, scene=scene, scenes=[scene, scene2], target=target, pixel=pixel, delta=deltas, kinds=kinds,
             targeted=target[:, 0] >= 0)
    _CASES[variant] = c
    return c


def census(fwd, c):
    """What a forward of c["scene"] (float32 means2D, conic_opacity, final_T) says about the targets: margin = the targeted tile's
    largest float32 power minus the cut -log(255 o), the transmittance left at the pixel it is reached at, the boxes' sizes."""
    m2, co = fwd["means2D"].astype(F), fwd["conic_opacity"].astype(F)
    ids = np.nonzero(c["targeted"])[0]
    margin = np.empty(len(ids))
    T = np.empty(len(ids))
    for n, i in enumerate(ids):
        tx0, ty0, b, pix = tile_best_powers(m2, co, i)
        ix, iy = c["target"][i, 0] - tx0, c["target"][i, 1] - ty0
        margin[n] = float(b[iy, ix]) + math.log(255.0 * float(co[i, 3]))
        T[n] = fwd["final_T"][pix[iy, ix, 1], pix[iy, ix, 0]]
    cols, rows = box_tiles(m2, co, co[:, 3])
    vis = fwd["radii"] > 0
    m = np.asarray(fwd["means2D"], np.float64)
    centre = np.floor(m[ids] / 16.0).astype(int)
    return dict(targets=len(ids), visible=int(vis.sum()), diagonal=int((c["target"][ids] != centre).all(1).sum()),
                just_in=int(((margin >= 0) & (margin < 2e-4)).sum()), just_out=int(((margin < 0) & (margin > -2e-4)).sum()),
                hair=int((np.abs(margin) < 2e-5).sum()), closest=float(np.abs(margin).min()),
                blended=float((T > 0.5).mean()),
                rows_8=int((vis & (rows == 8) & (cols <= 15)).sum()), rows_9=int((vis & (rows == 9)).sum()),
                cols_15=int((vis & (cols == 15) & (rows <= 8)).sum()), cols_16=int((vis & (cols == 16)).sum()),
                off_image=int((vis & ((m[:, 0] < -0.5) | (m[:, 1] < -0.5) | (m[:, 0] > W - 0.5) | (m[:, 1] > H - 0.5))).sum()),
                border=int((vis & ((m[:, 0] < 16) | (m[:, 1] < 16) | (m[:, 0] >= 16 * (GX - 1)) | (m[:, 1] >= 16 * (GY - 1)))).sum()),
                ratio_above_4=int((_axis_ratio2(co[vis]) > 16.0).sum()), ratio_above_8=int((_axis_ratio2(co[vis]) > 64.0).sum()))


def _axis_ratio2(co):
    """lambda_max / lambda_min of the conics (= of the covariances)"""
    A, B, C = (co[:, k].astype(np.float64) for k in range(3))
    mid, d = 0.5 * (A + C), np.sqrt(np.maximum(0.25 * (A - C) ** 2 + B * B, 0.0))
    return (mid + d) / np.maximum(mid - d, 1e-300)


def emitted_boxes(keys, vals, n):
    """From a view's sorted lists (keys: tile << 32 | depth bits; vals: Gaussian ids): per Gaussian the number of tiles it emitted and
    the columns and rows of their bounding box."""
    tile = (np.asarray(keys).view(np.uint64) >> np.uint64(32)).astype(np.int64)
    ids = np.asarray(vals).view(np.uint32).astype(np.int64)
    tx, ty = tile % GX, tile // GX
    count = np.bincount(ids, minlength=n)
    big = 1 << 20
    x0, x1, y0, y1 = np.full(n, big), np.full(n, -1), np.full(n, big), np.full(n, -1)
    np.minimum.at(x0, ids, tx)
    np.maximum.at(x1, ids, tx)
    np.minimum.at(y0, ids, ty)
    np.maximum.at(y1, ids, ty)
    has = count > 0
    return count, np.where(has, x1 - x0 + 1, 0), np.where(has, y1 - y0 + 1, 0)
