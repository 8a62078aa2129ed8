"""The host reference of gsr_contrib_stats (csrc/contrib_stats.hip), the checker that holds library outputs to it, and the seeded cases
of tests/test_gpu_contrib_stats.py.  Importable without a GPU (tests/test_cpu_contrib_ref.py).

Sums: the plain-C oracle as it stands.  forward_backward(scene, dL_dpix, exact=True) on a colors_precomp scene returns dL_dcolor[:, c]
= sum over pixels of w dL_dpix[c], w = alpha T, in float64 with the oracle's bit-exact decisions: channel 0 = ones is the weight_sum
reference, channel 1 = the cleaned weight map the weighted one.  One call per view, added up.

Maximum and counts: walk(), a numpy restatement of the compositing walk over the oracle's own forward state (vals, ranges, means2D,
conic_opacity).  power and the T recurrence are float32 with the written operation order of power_exact and the forward (numpy float32
rounds once per operation, like the kernels); exp is evaluated in float64 and rounded to float32 -- the device's may differ from that by
an ulp -- so a decision at a cut (alpha < 1/255, T (1 - alpha) < 1e-4) is UNCERTAIN when the value lies within a relative
(c + 2) 2^-22 of the cut, c = the contributions so far at the pixel (the ulp budget of exp, the opacity product and the T chain).  From
its first uncertain decision on a pixel is uncertain: whichever way that decision goes, T and with it every later decision and weight
at the pixel may differ, so every later entry (and the entry of the decision itself) that could reach the alpha cut is a POSSIBLE
contribution with a weight of at most alpha times the T at that point (T never grows).  (The alpha cut is treated like the stop cut in
this: an entry that is blended or not changes T behind it by 0.4 %.)  Per Gaussian this gives brackets lo <= . <= hi for pixel_count,
weight_max and dominant_count; at a certain pixel i is the certain winner only if it beats every other entry by more than the band.

Bars (derived, not measured), L = the longest tile list of the case:
  pixel_count, dominant_count   inside their brackets (equal where lo == hi)
  weight_max                    inside [max_lo (1 - e), max_hi (1 + e)], e = (L + 4) 2^-24
  weight_sum                    |got - ref| <= (n_i + L + 5) 2^-24 ref per Gaussian, n_i = count_hi: float32 summation of n non-negative
                                terms in any order plus the per-term chain; a Gaussian with possible contributions gets their weights on
                                top (the oracle's decision there may be the other one)
  sum_i weight_sum (no map)     = sum over pixels of 1 - final_T of the oracle, within the sum of the per-Gaussian bars plus the
                                T chain's (L + 5) 2^-24 of it
CAP: in every case at most 2 % of the visible Gaussians may have lo != hi in any bracket (tests/test_cpu_contrib_ref.py asserts it on
the reference alone), so that wide brackets cannot hide a failure."""
import functools

import numpy as np

F = np.float32
NAMES = ("weight_sum", "weight_max", "pixel_count", "dominant_count")
CAP = 0.02
BAND = 2.0 ** -22
CUT_A = F(1.0) / F(255.0)
CUT_T = F(0.0001)


def clean_map(m):
    """the weight map as the kernel reads it: values with !(m > 0) -- negative, zero, NaN -- are 0"""
    m = np.asarray(m, F)
    with np.errstate(invalid="ignore"):
        return np.where(m > 0, m, F(0)).astype(F)


def walk(fwd, W, H, m=None):
    """fwd: a forward state (P, vals, ranges [T,2], means2D [P,2], conic_opacity [P,4]); m: [H,W] weight map or None.  Returns a dict of
    per-Gaussian arrays: count_lo/hi, dom_lo/hi (int64), max_lo/hi (float64 of float32 products w m), sum (float64, the nominal walk's
    sum of w m), slack (float64: the possible contributions' weights), and L, the longest list."""
    P = int(fwd["P"])
    gx, gy = (W + 15) // 16, (H + 15) // 16
    out = dict(count_lo=np.zeros(P, np.int64), count_hi=np.zeros(P, np.int64), dom_lo=np.zeros(P, np.int64), dom_hi=np.zeros(P, np.int64),
               max_lo=np.zeros(P), max_hi=np.zeros(P), sum=np.zeros(P), slack=np.zeros(P), L=0)
    if P == 0:
        return out
    vals, ranges = np.asarray(fwd["vals"]).astype(np.int64), np.asarray(fwd["ranges"]).astype(np.int64).reshape(-1, 2)
    m2, co = np.asarray(fwd["means2D"], F), np.asarray(fwd["conic_opacity"], F)
    mm_img = np.ones((H, W), F) if m is None else clean_map(m)
    lx, ly = np.tile(np.arange(16), 16), np.repeat(np.arange(16), 16)
    for t in range(gx * gy):
        a, b = ranges[t]
        n = int(b - a)
        if n <= 0:
            continue
        out["L"] = max(out["L"], n)
        ids = vals[a:b]
        px, py = (t % gx) * 16 + lx, (t // gx) * 16 + ly
        inside = (px < W) & (py < H)
        mm = np.where(inside, mm_img[np.minimum(py, H - 1), np.minimum(px, W - 1)], F(0)).astype(F)
        pxf, pyf = px.astype(F), py.astype(F)
        T = np.ones(256, F)
        done = ~(inside & (mm > 0))
        unc = np.zeros(256, bool)
        Tunc = np.zeros(256, F)
        c = np.zeros(256, np.int64)
        Wn, Wall, U = np.zeros((n, 256), F), np.zeros((n, 256), F), np.zeros((n, 256), F)
        for e in range(n):
            i = ids[e]
            x, y = m2[i]
            A, B, C, o = co[i]
            dx, dy = x - pxf, y - pyf
            with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                power = F(-0.5) * (A * dx * dx + C * dy * dy) - B * dx * dy
                ex = np.exp(power.astype(np.float64)).astype(F)
                alpha = np.minimum(F(0.99), o * ex)
                test = T * (F(1) - alpha)
            band = (c + 2) * BAND
            pos = power > 0
            a_lt = alpha < CUT_A
            a_unc = np.abs(alpha.astype(np.float64) - float(CUT_A)) <= band * float(CUT_A)
            s_lt = test < CUT_T
            s_unc = np.abs(test.astype(np.float64) - float(CUT_T)) <= band * float(CUT_T)
            # the nominal walk
            cnt = ~done & ~pos & ~a_lt
            stop = cnt & s_lt
            hit = cnt & ~stop
            w = np.where(hit, alpha * T, F(0)).astype(F)
            Wall[e] = w
            # where a decision of this entry is uncertain on a pixel that was certain so far
            new_unc = ~done & ~unc & ~pos & (a_unc | (~a_lt & s_unc))
            Wn[e] = np.where(hit & ~unc & ~new_unc, w, F(0))
            pot = (unc | new_unc) & ~pos & (alpha.astype(np.float64) >= float(CUT_A) * (1 - band))
            U[e] = np.where(pot, alpha * np.where(unc, Tunc, T), F(0))
            Tunc = np.where(new_unc, T, Tunc)
            unc |= new_unc
            T = np.where(hit, test, T)
            done |= stop
            c += hit
        sure, poss = Wn > 0, U > 0
        out["count_lo"][ids] += sure.sum(1)
        out["count_hi"][ids] += (sure | poss).sum(1)
        wm_lo = (Wn * mm[None, :]).max(1).astype(np.float64)
        wm_hi = np.maximum(wm_lo, (U * mm[None, :]).max(1).astype(np.float64))
        out["max_lo"][ids] = np.maximum(out["max_lo"][ids], wm_lo)
        out["max_hi"][ids] = np.maximum(out["max_hi"][ids], wm_hi)
        out["sum"][ids] += (Wall.astype(np.float64) * mm[None, :].astype(np.float64)).sum(1)
        out["slack"][ids] += (U.astype(np.float64) * mm[None, :].astype(np.float64)).sum(1)
        # dominance: the candidates of a pixel are the entries within the band of its largest certain weight, and the possible ones
        # that could get there; a single certain candidate is the certain winner
        best = Wn.max(0).astype(np.float64)
        thr = best * (1 - (c + 2) * BAND)
        cand_sure = sure & (Wn >= thr[None, :])
        cand = cand_sure | (poss & (U >= thr[None, :]))
        single = (cand.sum(0) == 1) & (cand_sure.sum(0) == 1)
        out["dom_lo"][ids] += (cand & single[None, :]).sum(1)
        out["dom_hi"][ids] += cand.sum(1)
    return out


def hand_values(fwd, W, H):
    """pure-Python float64 restatement for the hand cases (lists of one tile, no cut anywhere near): per Gaussian (sum, max, count,
    dominant) from alpha = min(0.99, o exp(power)) and the T product, pixel by pixel"""
    import math
    P = int(fwd["P"])
    res = [[0.0, 0.0, 0, 0] for _ in range(P)]
    ranges = np.asarray(fwd["ranges"]).reshape(-1, 2)
    gx = (W + 15) // 16
    for y in range(H):
        for x in range(W):
            a, b = ranges[(y // 16) * gx + x // 16]
            T, best, who = 1.0, 0.0, -1
            for k in range(int(a), int(b)):
                i = int(fwd["vals"][k])
                mx, my = (float(v) for v in fwd["means2D"][i])
                A, B, C, o = (float(v) for v in fwd["conic_opacity"][i])
                dx, dy = mx - x, my - y
                power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
                if power > 0:
                    continue
                alpha = min(0.99, o * math.exp(power))
                if alpha < 1.0 / 255.0:
                    continue
                if T * (1 - alpha) < 1e-4:
                    break
                w = alpha * T
                r = res[i]
                r[0] += w
                r[1] = max(r[1], w)
                r[2] += 1
                if w > best:
                    best, who = w, i
                T *= 1 - alpha
            if who >= 0:
                res[who][3] += 1
    return res


# ---- the reference of a case ------------------------------------------------------------------------------------------------------
def reference(scenes, weights=None, oracle=None):
    """scenes: one colors_precomp oracle Scene per view; weights: [V,H,W] or None.  Returns a dict: sum / sum_plain (float64 [P], the
    oracle's weighted / unweighted sums), walk_sum (the restatement's nominal weighted sum), slack, count_lo/hi, dom_lo/hi, max_lo/hi,
    L, visible (bool [P]), opacity_sum (sum over pixels and views of 1 - final_T), uncertain (bool [P]: lo != hi in some bracket)."""
    from oracle.oracle import Oracle
    orc = oracle or Oracle()
    s0 = scenes[0]
    P, W, H = s0.P, s0.W, s0.H
    ref = dict(sum=np.zeros(P), sum_plain=np.zeros(P), walk_sum=np.zeros(P), slack=np.zeros(P), count_lo=np.zeros(P, np.int64),
               count_hi=np.zeros(P, np.int64), dom_lo=np.zeros(P, np.int64), dom_hi=np.zeros(P, np.int64), max_lo=np.zeros(P),
               max_hi=np.zeros(P), L=0, visible=np.zeros(P, bool), opacity_sum=0.0, fwd=[])
    for v, s in enumerate(scenes):
        assert s.colors_precomp is not None, "the sums come out of the oracle's dL_dcolor: colors_precomp scenes only"
        m = None if weights is None else clean_map(weights[v])
        dL = np.zeros((3, H, W), F)
        dL[0] = 1
        dL[1] = 1 if m is None else m
        fwd, g = orc.forward_backward(s, dL, exact=True)
        ref["fwd"].append(fwd)
        if P == 0:
            continue
        ref["sum_plain"] += g["exact"]["dL_dcolor"][:, 0]
        ref["sum"] += g["exact"]["dL_dcolor"][:, 1]
        ref["visible"] |= np.asarray(fwd["radii"]) > 0
        ref["opacity_sum"] += float((1.0 - fwd["final_T"].astype(np.float64)).sum())
        wk = walk(fwd, W, H, m)
        for k in ("count_lo", "count_hi", "dom_lo", "dom_hi", "slack"):
            ref[k] += wk[k]
        ref["walk_sum"] += wk["sum"]
        ref["max_lo"] = np.maximum(ref["max_lo"], wk["max_lo"])
        ref["max_hi"] = np.maximum(ref["max_hi"], wk["max_hi"])
        ref["L"] = max(ref["L"], wk["L"])
    ref["uncertain"] = (ref["count_lo"] != ref["count_hi"]) | (ref["dom_lo"] != ref["dom_hi"]) | (ref["max_lo"] != ref["max_hi"])
    return ref


def uncertain_fraction(ref):
    vis = int(ref["visible"].sum())
    return (int((ref["uncertain"] & ref["visible"]).sum()) / vis) if vis else 0.0


def sum_bar(ref, base=None, more_terms=0):
    """per-Gaussian bound on |weight_sum - ref|: (n_i + L + 5) 2^-24 ref + the possible contributions' weights; more_terms: terms of
    the float32 sum beyond the contributions (the caller's running value under accumulate)"""
    base = ref["sum"] if base is None else base
    return (ref["count_hi"] + more_terms + ref["L"] + 5) * 2.0 ** -24 * np.abs(base) + ref["slack"]


def check(out, ref, tag="", old=None, weighted=True):
    """Hold library outputs (a dict with any of NAMES as numpy arrays) to reference(...)'s result.  old: the caller's running values
    (dict, accumulate = 1) the call started from; weighted=False: the call had no weight map although the reference has one."""
    assert any(k in out for k in NAMES), "nothing to check"
    P = ref["count_lo"].shape[0]
    z = dict(weight_sum=np.zeros(P, F), weight_max=np.zeros(P, F), pixel_count=np.zeros(P, np.int32), dominant_count=np.zeros(P, np.int32))
    old = z if old is None else old
    for k, lo, hi in (("pixel_count", "count_lo", "count_hi"), ("dominant_count", "dom_lo", "dom_hi")):
        if k in out:
            a = np.asarray(out[k])
            assert a.dtype == np.int32 and a.shape == (P,), (tag, k, a.dtype, a.shape)
            d = a.astype(np.int64) - np.asarray(old[k]).astype(np.int64)
            bad = np.nonzero((d < ref[lo]) | (d > ref[hi]))[0]
            assert bad.size == 0, "%s %s: %d rows outside their bracket, first %d: %d not in [%d, %d]" % (
                tag, k, bad.size, bad[0], d[bad[0]], ref[lo][bad[0]], ref[hi][bad[0]])
    e = (ref["L"] + 4) * 2.0 ** -24
    if "weight_max" in out:
        a = np.asarray(out["weight_max"])
        assert a.dtype == np.float32 and a.shape == (P,), (tag, a.dtype, a.shape)
        o = np.asarray(old["weight_max"]).astype(np.float64)
        lo, hi = np.maximum(o, ref["max_lo"] * (1 - e)), np.maximum(o, ref["max_hi"] * (1 + e))
        bad = np.nonzero(~((a >= lo) & (a <= hi)))[0]
        assert bad.size == 0, "%s weight_max: %d rows outside [max_lo (1 - e), max_hi (1 + e)], first %d: %.9g not in [%.9g, %.9g]" % (
            tag, bad.size, bad[0], a[bad[0]], lo[bad[0]], hi[bad[0]])
    if "weight_sum" in out:
        a = np.asarray(out["weight_sum"])
        assert a.dtype == np.float32 and a.shape == (P,), (tag, a.dtype, a.shape)
        base = ref["sum"] if weighted else ref["sum_plain"]
        o = np.asarray(old["weight_sum"]).astype(np.float64)
        want = o + base
        bar = sum_bar(ref, want, 0 if old is z else 1)   # (accumulate: the old value is one more non-negative term of the float32 sum)
        err = np.abs(a.astype(np.float64) - want)
        bad = np.nonzero(~(err <= bar))[0]
        assert bad.size == 0, "%s weight_sum: %d rows outside the bar, worst %.3g x its bar (row %d: %.9g vs %.9g)" % (
            tag, bad.size, (err[bad] / np.maximum(bar[bad], 1e-300)).max(), bad[0], a[bad[0]], want[bad[0]])
    return e


def check_total(weight_sum, ref, tag=""):
    """sum_i weight_sum (no weight map, accumulate = 0) against the oracle's sum over pixels of 1 - final_T"""
    got = float(np.asarray(weight_sum, np.float64).sum())
    bar = float(sum_bar(ref, ref["sum_plain"]).sum()) + (ref["L"] + 5) * 2.0 ** -24 * ref["opacity_sum"]
    assert abs(got - ref["opacity_sum"]) <= bar, "%s: sum_i weight_sum = %.9g, sum (1 - final_T) = %.9g, bar %.3g" % (
        tag, got, ref["opacity_sum"], bar)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def _flat(P, xy, z, scale, opacity, seed):
    """P axis-aligned Gaussians at screen positions xy (fractions of the half image) and depths z"""
    rng = np.random.default_rng(seed)
    xy, z = np.asarray(xy, np.float64).reshape(P, 2), np.asarray(z, np.float64).reshape(P)
    t = np.tan(np.radians(30.0))
    means = np.stack([xy[:, 0] * t * z, xy[:, 1] * t * z, z], 1).astype(F)
    return dict(means3D=means, scales=np.broadcast_to(np.asarray(scale, F), (P, 3)).copy(),
                rotations=np.tile(np.array([1, 0, 0, 0], F), (P, 1)), opacities=np.broadcast_to(np.asarray(opacity, F), (P, 1)).copy(),
                colors_precomp=rng.uniform(0, 1, (P, 3)).astype(F), shs=(0.5 * rng.standard_normal((P, 4, 3))).astype(F), sh_degree=1)


def _views(g, poses, W, H, **kw):
    import camera_cases as CC
    kw.setdefault("mode", "colors")
    return CC.views_of(g, poses, W, H, **kw)


def _eye():
    import torch
    return torch.eye(4)


def cloud(name):
    """(Gaussian dict, poses, W, H) of a named case"""
    import camera_cases as CC
    from pcrender import synth
    rng = np.random.default_rng(5)
    if name == "one":                  # one Gaussian on one tile
        return _flat(1, [[0.1, -0.2]], [2.0], [0.25, 0.15, 0.2], 0.7, 1), [_eye()], 16, 16
    if name == "two":                  # two overlapping, the nearer one first in the list
        return _flat(2, [[0.1, -0.2], [-0.15, 0.1]], [2.0, 2.5], [[0.25, 0.15, 0.2], [0.3, 0.3, 0.3]], [[0.7], [0.5]], 2), [_eye()], 16, 16
    if name == "partial_17x16":        # a second tile column one pixel wide
        return _flat(40, rng.uniform(-0.9, 0.9, (40, 2)), rng.uniform(1.5, 3.0, 40), 0.12, rng.uniform(0.2, 0.8, (40, 1)), 3), [_eye()], 17, 16
    if name == "partial_40x24":        # partial tiles in both directions, and one Gaussian that covers all six tiles
        g = _flat(60, rng.uniform(-0.9, 0.9, (60, 2)), rng.uniform(1.5, 3.0, 60), 0.1, rng.uniform(0.2, 0.8, (60, 1)), 4)
        g["means3D"][0] = [0.02, -0.01, 1.2]
        g["scales"][0] = 1.5
        g["opacities"][0] = 0.3
        return g, [_eye()], 40, 24
    if name == "stack300":             # a list longer than four staging rounds, no pixel ever stops
        return _flat(300, rng.uniform(-0.3, 0.3, (300, 2)), np.linspace(1.5, 3.0, 300), 0.3, 0.02, 5), [_eye()], 16, 16
    if name == "opaque70":             # 70 wide splats of opacity 0.99 centred in one quadrant: alpha is 0.99 exp(power) with power > -0.02
        # all over the tile, two entries are blended (T = 0.01.., 1.0e-4..), the third stops every pixel, 67 get exact zeros
        return _flat(70, -0.5 + rng.uniform(-0.2, 0.2, (70, 2)), np.linspace(1.5, 3.0, 70), 30.0, 0.99, 6), [_eye()], 16, 16
    if name == "behind":               # behind the camera, off screen, and a few in view
        g = CC.mixed_cloud(0, seed=12, P=200)
        return g, [CC.pose(3)], 70, 50
    if name == "views3":               # three distinct cameras
        return CC.cloud(400, 41, 1, scale=(0.1, 0.3)), [CC.pose(3), CC.pose(4), CC.pose(7)], 70, 50
    if name == "random2000":
        return synth.random_scene(2000, 130, 35, seed=19, sh_degree=1), [_eye()], 130, 35
    raise KeyError(name)


CASES = ("one", "two", "partial_17x16", "partial_40x24", "stack300", "opaque70", "behind", "views3", "random2000")
WEIGHTED = ("views3_mask", "views3_random")


def weight_map(name, V, W, H):
    """[V,H,W] float32: a 0/1 mask with the first quadrant of every view's first tile (and a random tenth) zero, or random values in
    [0, 1] with a few negatives and a NaN"""
    rng = np.random.default_rng(23)
    if name == "views3_mask":
        m = (rng.uniform(0, 1, (V, H, W)) > 0.1).astype(F)
        m[:, :8, :8] = 0
        return m
    m = rng.uniform(0, 1, (V, H, W)).astype(F)
    m[:, 3::7, 5::11] = -0.5
    m[0, 20, 30] = np.nan
    m[V - 1, 2, 2] = np.nan
    return m


def build(name, **kw):
    """(scenes, weights or None) of a case; kw goes to util.scene_from (mode, use_cov3d)"""
    base = name if name in CASES else "views3"
    g, poses, W, H = cloud(base)
    return _views(g, poses, W, H, **kw), (None if name in CASES else weight_map(name, len(poses), W, H))


@functools.lru_cache(maxsize=None)
def case(name, use_cov3d=False):
    """dict(scenes, weights, ref) of a case; computed once, shared by the tests, not modified"""
    scenes, weights = build(name, use_cov3d=use_cov3d)
    return dict(scenes=scenes, weights=weights, ref=reference(scenes, weights))
