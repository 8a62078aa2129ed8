"""Scenes for the once-per-round code of the render kernels (gathers, footprint test, staging of the survivors in groups), and
a CPU model of the backward's rounds that says which situations a scene really produces.  Test infrastructure, shared by
tests/test_gpu_round_overhead.py (which renders the scenes) and tests/test_cpu_round_cases.py (which checks, with the oracle, that
the scenes do what they are for).

All scenes are 64 x 48 pixels (4 x 3 tiles, 8 x 6 quadrants) with at most 3 000 Gaussians, given in pixel space: centre, two
sigmas, an in-plane angle, opacity; the index is the depth order.  Two cameras (the second one a few centimetres to the side) make
them batches.

  scatter   small anisotropic splats all over the image and up to 12 pixels outside it: centres inside, beside and diagonal to
            every quadrant, lists of several rounds per tile.
  front     the same behind a front of nearly opaque blobs: pixels terminate at different depths, so the forward's live boxes shrink
            while it walks and the backward's rounds see boxes of every size.
  long      one tile with more than 1 024 entries of opacity 0.0045 .. 0.008 that no pixel terminates on: three slices at V = 1,
            two at V = 2, incomplete last groups at slice boundaries.
  sparse    one tile whose list is 800 pixel-sized splats inside ONE quadrant plus a handful in the others: the other quadrants'
            rounds keep zero to two survivors (rounds without a survivor, groups of one), the first quadrant's rounds keep all 64.
            At the back of the list a faint line along a pixel row, one along a column and a dot: live boxes of one row, one
            column, one pixel.
"""
import numpy as np

import util

W, H = 64, 48
F = np.float32
Z0 = 2.5
NAMES = ("scatter", "front", "long", "sparse")


def cameras():
    a = util.identity_camera(W, H, 60.0)
    c2w = np.eye(4, dtype=np.float32)
    c2w[0, 3] = 0.03
    return [a, util._view_arrays(c2w, W, H, 60.0)]


def _cloud(px, py, s1, s2, ang, op, rng):
    """pixel-space splats -> a cloud seen by the first camera; index = depth order"""
    K = len(px)
    view = cameras()[0]
    pm = np.asarray(view["projmatrix"], np.float64).reshape(4, 4)
    kx, ky = 0.5 * W * pm[0, 0], 0.5 * H * pm[1, 1]
    z = Z0 + 0.002 * np.arange(K)
    means = np.stack([(px - (W - 1) / 2) / kx * z, (py - (H - 1) / 2) / ky * z, z], 1).astype(F)
    fx = W / (2.0 * view["tanfovx"])
    sc = np.stack([s1 * z / fx, s2 * z / fx, 0.2 * np.minimum(s1, s2) * z / fx], 1)
    q = np.stack([np.cos(ang / 2), np.zeros(K), np.zeros(K), np.sin(ang / 2)], 1)
    return dict(means3D=means, scales=sc.astype(F), rotations=q.astype(F), opacities=np.asarray(op, F).reshape(K, 1),
                shs=(0.5 * rng.standard_normal((K, 4, 3))).astype(F), sh_degree=1)


def _scatter(rng, K, lo=0.6, hi=3.0):
    return (rng.uniform(-12, W + 12, K), rng.uniform(-12, H + 12, K), rng.uniform(lo, hi, K), rng.uniform(lo, hi, K) * rng.uniform(0.3, 1.0, K),
            rng.uniform(0, np.pi, K), rng.uniform(0.05, 0.9, K))


def cloud(name):
    rng = np.random.default_rng({"scatter": 11, "front": 12, "long": 13, "sparse": 14}[name])
    if name == "scatter":
        parts = [_scatter(rng, 1500)]
    elif name == "front":
        K = 100
        blobs = (rng.uniform(0, W, K), rng.uniform(0, H, K), rng.uniform(3, 9, K), rng.uniform(3, 9, K), rng.uniform(0, np.pi, K),
                 rng.uniform(0.9, 1.0, K))
        parts = [_scatter(rng, 150), blobs, _scatter(rng, 1400)]
    elif name == "long":
        K = 1300
        stack = (rng.uniform(15, 32, K), rng.uniform(15, 32, K), rng.uniform(1.5, 7, K), rng.uniform(1.5, 7, K), rng.uniform(0, np.pi, K),
                 rng.uniform(0.0045, 0.008, K))
        parts = [stack, _scatter(rng, 120)]
    else:
        K = 800
        tiny = [rng.uniform(32, 40, K), rng.uniform(16, 24, K), rng.uniform(0.45, 0.7, K), rng.uniform(0.45, 0.7, K), rng.uniform(0, np.pi, K),
                rng.uniform(0.02, 0.1, K)]
        # a handful in the tile's other three quadrants at random depth ranks, and at the very back of the list -- behind 80 entries
        # that stay inside the first quadrant -- a thin horizontal line, a thin vertical line and a dot, one per quadrant, faint
        # enough (opacity 0.012) to reach 1/255 in a single pixel row / column / pixel: the deepest round of each of those quadrants
        # has exactly that live box
        where = np.concatenate([rng.choice(K - 83, 16, replace=False), [K - 3, K - 2, K - 1]])
        quad = np.concatenate([rng.integers(1, 4, 16), [1, 2, 3]])
        tiny[0][where] = 32 + 8 * (quad & 1) + rng.uniform(1, 7, 19)
        tiny[1][where] = 16 + 8 * (quad >> 1) + rng.uniform(1, 7, 19)
        tiny[5][where] = rng.uniform(0.3, 0.6, 19)
        for k, (x, y, s1, s2) in enumerate([(44.0, 19.0, 3.0, 0.2), (35.0, 28.0, 0.2, 3.0), (45.0, 29.0, 0.2, 0.2)]):
            i = K - 3 + k
            tiny[0][i], tiny[1][i], tiny[2][i], tiny[3][i], tiny[4][i], tiny[5][i] = x, y, s1, s2, 0.0, 0.012
        parts = [_scatter(rng, 100), tuple(tiny)]
    cols = [np.concatenate([p[k] for p in parts]) for k in range(6)]
    return _cloud(*cols, rng)


def scenes(name, V):
    g = cloud(name)
    return [util.scene_from(g, v, W, H, bg=(0.2, 0.1, 0.3)) for v in cameras()[:V]]


# ---------------------------------------------------------------------------------------------------- the backward's rounds
def may_touch_rect(mx, my, A, B, C, o, x0, y0, x1, y1):
    """csrc/tile_cull.hpp may_touch_rect on float32 arrays (one rounding per operation; host forms of rcp and log2)"""
    with np.errstate(all="ignore"):
        f = lambda v: np.asarray(v, F)  # noqa: E731
        mx, my, A, B, C, o = (f(v) for v in (mx, my, A, B, C, o))
        x0, y0, x1, y1 = F(x0), F(y0), F(x1), F(y1)
        clamp = lambda v, lo, hi: np.fmin(np.fmax(v, lo), hi)  # noqa: E731
        thr = F(-0.6931471805599453) * np.log2(F(255.0) * o).astype(F)
        dxl, dxh, dyl, dyh = mx - x1, mx - x0, my - y1, my - y0
        ex, ey = clamp(F(0), dxl, dxh), clamp(F(0), dyl, dyh)
        yy = clamp(-B * (F(1) / C) * ex, dyl, dyh)
        m = F(-0.5) * (A * ex * ex + C * yy * yy) - B * ex * yy
        xx = clamp(-B * (F(1) / A) * ey, dxl, dxh)
        m = np.fmax(m, F(-0.5) * (A * xx * xx + C * ey * ey) - B * xx * ey)
        ax, ay = np.fmax(np.abs(dxl), np.abs(dxh)), np.fmax(np.abs(dyl), np.abs(dyh))
        E = F(1e-5) * (A * ax * ax + C * ay * ay + np.abs(B) * ax * ay) + F(1e-4) + F(1e-5) * np.abs(thr)
        keep = ~(m + E < thr)
        keep = np.where(~((A > 0) & (C > 0) & (A * C - B * B > 0)), True, keep)
        return np.where(o <= 0, False, keep)


def backward_rounds(fwd, V):
    """The rounds k_render_backward walks for one view with the lists of `fwd` (an oracle / reference forward: the library's own lists
    when it runs with the reference's full lists), and what the footprint test leaves of each: a dict of counts.
      residue[r]          rounds whose survivor count is r mod 4 (r != 0: the round's last group of four is padded), survivors > 0
      empty               rounds with live pixels and no survivor
      full                rounds in which all 64 entries survive
      last_inner_slice    rounds that end a slice at a boundary inside the list (the next item starts from the forward's checkpoint)
      box_pixel / box_row / box_column
                          rounds whose live box is a single pixel / one row / one column
      region[k]           tested entries by where their centre lies relative to the live box, k = 3 (y: above, within, below) + x
      items, slices_max   work items walked, the largest number of slices of one tile
      staged, groups      survivors, groups of four evaluated (4 groups - staged = padded places)"""
    from batch_cases import slice_length
    S = slice_length(V)
    gx = (W + 15) // 16
    m2, co = fwd["means2D"].astype(F), fwd["conic_opacity"].astype(F)
    out = dict(residue=[0, 0, 0, 0], empty=0, full=0, last_inner_slice=0, box_pixel=0, box_row=0, box_column=0, region=[0] * 9, items=0,
               slices_max=0, groups=0, staged=0)
    for t, (r0, r1) in enumerate(fwd["ranges"]):
        ids = fwd["vals"][int(r0):int(r1)].astype(np.int64)
        ty, tx = divmod(t, gx)
        for q in range(4):
            x0, y0 = tx * 16 + (q & 1) * 8, ty * 16 + (q >> 1) * 8
            ys, xs = np.meshgrid(np.arange(y0, y0 + 8), np.arange(x0, x0 + 8), indexing="ij")
            inside = (ys < H) & (xs < W)
            last = np.where(inside, fwd["n_contrib"][np.minimum(ys, H - 1), np.minimum(xs, W - 1)], 0).astype(np.int64)
            total = int(last.max())
            nslices = 0
            for chunk in range(32):
                lo = chunk * S
                if lo >= total:
                    break
                last_chunk = chunk == 31 or lo + S >= total
                hi0 = total if last_chunk else lo + S
                out["items"] += 1
                nslices += 1
                for hi in range(hi0, lo, -64):
                    round_lo = max(hi - 64, lo)
                    live = last > round_lo
                    if not live.any():
                        continue
                    yy, xx = np.nonzero(live)
                    bx0, bx1, by0, by1 = x0 + xx.min(), x0 + xx.max(), y0 + yy.min(), y0 + yy.max()
                    out["box_pixel"] += int(bx0 == bx1 and by0 == by1)
                    out["box_row"] += int(by0 == by1 and bx0 != bx1)
                    out["box_column"] += int(bx0 == bx1 and by0 != by1)
                    e = ids[round_lo:hi]
                    cx, cy = m2[e, 0], m2[e, 1]
                    reg = 3 * (np.where(cy < by0, 0, np.where(cy > by1, 2, 1))) + np.where(cx < bx0, 0, np.where(cx > bx1, 2, 1))
                    for k in range(9):
                        out["region"][k] += int((reg == k).sum())
                    nsurv = int(may_touch_rect(cx, cy, co[e, 0], co[e, 1], co[e, 2], co[e, 3], bx0, by0, bx1, by1).sum())
                    out["staged"] += nsurv
                    out["groups"] += (nsurv + 3) >> 2
                    if nsurv:
                        out["residue"][nsurv & 3] += 1
                    out["empty"] += int(nsurv == 0)
                    out["full"] += int(nsurv == 64)
                    out["last_inner_slice"] += int(hi - 64 <= lo and not last_chunk)
            out["slices_max"] = max(out["slices_max"], nslices)
    return out
