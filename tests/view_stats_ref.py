"""The host reference of gsr_backward_view_stats (csrc/view_stats.hip), the checker that holds library outputs to it, and the seeded
scenes of tests/test_gpu_view_stats.py.  Importable without a GPU (tests/test_cpu_view_stats_ref.py).

The entry is a function of the per-view 64-B gradient records (words 0-1 mean2D, 5-7 colour, 8 opacity) and the forward's radii, and
both can be read back: the reference is fed with the LIBRARY'S OWN records, which isolates the new kernel from the render backward.

  reference(records [V,P,16], radii [V,P], old=None)   float64 numpy, views ascending
  check(out, ref)                                      integers exact, shares bit-equal, grad_norm_sum within 1 float32 ulp
  norm_gap(records, radii)                             how far sum_v |g_v| and |sum_v g_v| lie apart: the point of the entry
  cloud / poses / scenes                               the seeded scenes (opposite cameras, a view that sees nothing)"""
import numpy as np

F = np.float32
STATS = ("grad_norm_sum", "visible_views", "max_radius")
SHARES = ("mean2D", "color", "opacity")


def reference(records, radii, old=None):
    """records [V,P,16] float32, radii [V,P] integers; old: None (accumulate = 0) or the caller's running (grad_norm_sum float32 [P],
    visible_views [P], max_radius [P]) (accumulate = 1).  Returns a dict:
      grad_norm_sum64  float64 [P]: sum_v sqrt(gx^2 + gy^2), every term and the running sum in float64 from the float32 words, views
                       ascending, (+ float64(old)): the value BEFORE the one rounding to float32
      grad_norm_sum    that value rounded to float32
      visible_views, max_radius   int32 [P]
      mean2D [V,P,2], color [V,P,3], opacity [V,P]   the record words, float32 copies"""
    rec = np.asarray(records)
    assert rec.dtype == np.float32 and rec.ndim == 3 and rec.shape[2] == 16, (rec.dtype, rec.shape)
    rad = np.asarray(radii).astype(np.int64)
    V, P = rec.shape[:2]
    assert rad.shape == (V, P), rad.shape
    total = np.zeros(P, np.float64)
    for v in range(V):
        gx, gy = rec[v, :, 0].astype(np.float64), rec[v, :, 1].astype(np.float64)
        total = total + np.sqrt(gx * gx + gy * gy)
    vis = (rad > 0).sum(0)
    big = np.maximum(rad.max(0), 0)
    if old is not None:
        o_sum, o_vis, o_rad = old
        assert np.asarray(o_sum).dtype == np.float32
        total = np.asarray(o_sum).astype(np.float64) + total
        vis = np.asarray(o_vis).astype(np.int64) + vis
        big = np.maximum(np.asarray(o_rad).astype(np.int64), big)
    with np.errstate(over="ignore"):
        rounded = total.astype(np.float32)
    return dict(grad_norm_sum64=total, grad_norm_sum=rounded, visible_views=vis.astype(np.int32), max_radius=big.astype(np.int32),
                mean2D=rec[:, :, 0:2].copy(), color=rec[:, :, 5:8].copy(), opacity=rec[:, :, 8].copy())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(out, ref, tag=""):
    """Hold library outputs (a dict with any of STATS and SHARES as numpy arrays) to reference(...)'s result.  The integers are exact
    and the shares bit-equal (copies).  grad_norm_sum: the contract is ONE rounding of the float64 value to float32, which lies within
    half a float32 ulp of it; the kernel's float64 sqrt and additions may differ from numpy's in the last float64 bits (2^-29 of a
    float32 ulp), which can move a value that sits on a rounding boundary to the neighbouring float32: the bar is 1 float32 ulp of the
    float64 value, derived, not measured."""
    assert any(k in out for k in STATS + SHARES), "nothing to check"
    for k in ("visible_views", "max_radius"):
        if k in out:
            a = np.asarray(out[k])
            assert a.dtype == np.int32 and a.shape == ref[k].shape, (tag, k, a.dtype, a.shape)
            bad = np.nonzero(a != ref[k])[0]
            assert bad.size == 0, "%s %s: %d rows differ, first %d: %d != %d" % (tag, k, bad.size, bad[0], a[bad[0]], ref[k][bad[0]])
    for k in SHARES:
        if k in out:
            a = np.asarray(out[k])
            assert a.dtype == np.float32 and a.shape == ref[k].shape, (tag, k, a.dtype, a.shape)
            bad = np.argwhere(_bits(a) != _bits(ref[k]))
            assert bad.size == 0, "%s %s: %d words are not the records' bits, first at %s" % (tag, k, len(bad), tuple(bad[0]))
    if "grad_norm_sum" in out:
        a = np.asarray(out["grad_norm_sum"])
        x = ref["grad_norm_sum64"]
        assert a.dtype == np.float32 and a.shape == x.shape, (tag, a.dtype, a.shape)
        fin = np.isfinite(ref["grad_norm_sum"])
        assert np.isfinite(a[fin]).all(), "%s grad_norm_sum: not finite where the reference is" % tag
        ulp = np.spacing(np.abs(ref["grad_norm_sum"][fin])).astype(np.float64)
        err = np.abs(a[fin].astype(np.float64) - x[fin])
        bad = np.nonzero(err > ulp)[0]
        assert bad.size == 0, "%s grad_norm_sum: %d rows off by more than 1 float32 ulp, worst %.3g ulp" % (
            tag, bad.size, (err / ulp).max())
        assert (_bits(a[~fin]) == _bits(ref["grad_norm_sum"][~fin])).all(), "%s grad_norm_sum: overflow rows differ" % tag


def norm_gap(records, radii):
    """(rows, far): the Gaussians visible in two or more views, and those of them on which sum_v |g_v| and |sum_v g_v| differ by more
    than 1e-3 of the former, both in float64 from the records"""
    rec = np.asarray(records).astype(np.float64)
    sum_of_norms = np.sqrt(rec[:, :, 0] ** 2 + rec[:, :, 1] ** 2).sum(0)
    norm_of_sum = np.sqrt(rec[:, :, 0].sum(0) ** 2 + rec[:, :, 1].sum(0) ** 2)
    rows = (np.asarray(radii) > 0).sum(0) >= 2
    far = rows & (np.abs(sum_of_norms - norm_of_sum) > 1e-3 * sum_of_norms)
    return rows, far


# ---- scenes -----------------------------------------------------------------------------------------------------------------
W, H = 64, 48


def cloud(P, seed=71, degree=1):
    """camera_cases.cloud (depths 2..4 in front of the origin) with, from 16 Gaussians on, every 13th moved to z = -1: behind the
    cameras near the origin, in front of the opposite one"""
    import camera_cases as CC
    g = CC.cloud(P, seed, degree, scale=(0.1, 0.3))
    if P >= 16:
        g["means3D"][5::13, 2] = -1.0
    return g


def opposite():
    """H_c2w of a camera at z = 6 turned half a turn about y: it sees the cloud from behind, so a splat's screen-space gradient points
    the other way in x"""
    import torch
    Hc = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0]))
    Hc[2, 3] = 6.0
    return Hc


def poses(V, blind=False):
    """V cameras: near the origin looking down +z, the opposite one, and further ones near the origin; blind: view 1 looks away from
    the whole cloud (and the opposite camera moves to view 2)"""
    import camera_cases as CC
    out = [CC.pose(3), opposite(), CC.pose(4)] + [CC.pose(10 + k) for k in range(max(0, V - 3))]
    if blind:
        out.insert(1, CC.looking_away())
    return out[:V]


def scenes(P, V, blind=False, mode="sh", seed=71):
    import camera_cases as CC
    return CC.views_of(cloud(P, seed), poses(V, blind), W, H, mode=mode)


def dLs(scs, seed=500):
    import util
    return [util.seeded_dL(s, seed=seed + v) for v, s in enumerate(scs)]
