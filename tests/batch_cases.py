"""Seeded generator of VIEW-BATCH cases (gsr_forward_batch + gsr_backward_batch) for the batched sweep, and a host-side
prediction of the launch branches each case takes.  Importable without a GPU: numpy, pcrender.camera, pcrender.synth, util.

  case(i)      the Gaussians, a list of V views and what util.scene_from needs per view (scenes(c) builds the oracle Scenes)
  expected(i)  which V-dependent branches the case takes: the launch formulas of preprocess.hip (views per thread), sort.hip /
               api.hip (tile-sort passes, per-view depth-sort passes), render_bwd.hip (pulled work units, slice length), restated
  fingerprint  a hash of every byte of a case (the generator is deterministic)

Two classes.  small (i = 0 .. n-1): V from 2 to MAX_VIEWS, odd and sub-tile image sizes on both sides of the 255-tile boundary of
the tile sort, P at the edges of a wave / workgroup / slice, the options of test_gpu_fuzz._case, views from the reference caller's
circle path mixed with tilted cameras, views that see nothing, and near-planar slabs whose views need different depth-sort pass
counts.  medium (i = MEDIUM_BASE + j): (V, P) pairs that walk the views-per-thread ladder of k_preprocess, ragged last rows
included, on small images."""
import hashlib
import math

import numpy as np

import util
from pcrender import camera, synth

F = np.float32
MAX_VIEWS = 256                       # host.hpp
N_SMALL = 96
MEDIUM_BASE = 100000
# (V, P, W, H): vpt 4 rows 4+1 | vpt 8 rows 8+4 | vpt 2 exact | vpt = V | vpt 2 rows 2+2+2+1 | vpt 4 rows 4+4+4+1 | vpt 2 rows 8x2+1 |
# vpt 4 exact; one image with more than 255 tiles
MEDIUM = [(5, 300000, 64, 48), (12, 300000, 128, 96), (12, 100000, 96, 80), (3, 530000, 64, 64), (7, 180000, 80, 56),
          (13, 150000, 272, 256), (17, 70000, 112, 96), (8, 270000, 160, 112)]

VIEW_COUNTS = [2, 3, 4, 5, 7, 8, 12, 13, 16, 17, 31, 64, 256]
VIEW_WEIGHTS = [10, 10, 8, 10, 8, 8, 10, 8, 5, 5, 3, 3, 2]
SIZES_W = [1, 7, 16, 17, 33, 64, 97, 130, 200, 256, 331, 400, 512]
SIZES_H = [1, 5, 16, 23, 48, 65, 111, 144, 257, 300, 352]
POINTS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097, 12000]
FOVS = [30.0, 45.0, 60.0, 50.0]
SCALES = [0.004, 0.02, 0.05, 0.15, 0.4]
ANISOTROPY = [0.5, 1.0, 1.5]
# the first cases have some of their draws fixed, so that the census holds whatever the seeds give: the largest batch on a small
# image (pulled backward units by view count alone), 64 views of 704 tiles, slabs of mixed pass counts, empty first / middle / last
PINNED = {0: dict(V=256, W=256, H=144), 1: dict(V=64, W=512, H=352), 2: dict(V=12, W=130, H=111, P=1025, slab=True),
          3: dict(V=5, W=331, H=257, P=4097, slab=True), 4: dict(V=17, W=64, H=48, P=257, slab=True, empty=[16]),
          5: dict(V=13, slab=False, empty=[0, 6, 12])}


def ids(n_small=N_SMALL):
    return list(range(n_small)) + [MEDIUM_BASE + j for j in range(len(MEDIUM))]


def _np_view(v):
    """a camera.raster_settings_arrays dict with numpy members"""
    out = dict(v)
    for k in ("viewmatrix", "projmatrix", "campos"):
        out[k] = np.ascontiguousarray(np.asarray(v[k], dtype=F))
    return out


def _rot(axis, t):
    c, s = math.cos(t), math.sin(t)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def _camera(R, pos, W, H, fov):
    c2w = np.eye(4, dtype=F)
    c2w[:3, :3] = R.astype(F)
    c2w[:3, 3] = np.asarray(pos, F)
    return _np_view(util._view_arrays(c2w, W, H, fov))


def _far(view):
    """the camera pushed 50 units along its axis: every Gaussian lies behind the near plane (test_batch_edge_cases_vs_oracle)"""
    out = dict(view)
    out["viewmatrix"] = view["viewmatrix"].copy()
    out["viewmatrix"][3, 2] = -50.0
    return out


def _orbit(axis, theta, dist, W, H, fov, pivot=(0.0, 0.0, 2.0)):
    """a camera `dist` away from the pivot, turned by theta about `axis` and looking at the pivot (theta = 0, dist = 2: the identity
    camera, view-space z = z exactly)"""
    R = _rot(axis, theta)
    pos = np.asarray(pivot, np.float64) - dist * R[:, 2]
    if theta == 0.0:
        pos = np.round(pos)           # (0, 0, 0): no rounding residue in the translation
    return _camera(R, pos, W, H, fov)


# turn and distance of a slab view that needs 1 / 2 / 3 / 4 depth-sort passes (key spans below 2^8, 2^16, 2^24 codes and above)
SLAB_VIEWS = {1: (0.0, 2.0), 2: (0.001, 2.0), 3: (0.1, 2.0), 4: (1.3, 1.1)}


def _slab(g, fov, rng):
    """depth keys within 200 codes of 2.0 for the identity camera (util.build_scene depth_span_1), spread over its image"""
    P = g["means3D"].shape[0]
    span = 200
    base = (np.float32(2.0).view(np.uint32) - np.uint32(span // 2)) & np.uint32(0xFFFFFF00)
    z = (base + rng.integers(0, span, P).astype(np.uint32)).view(np.float32)
    z[:2] = np.array([base, base + np.uint32(span - 1)], np.uint32)[:min(P, 2)].view(np.float32)
    half = max(0.9 * 2.0 * math.tan(math.radians(fov) / 2), 1.0)
    g["means3D"][:, 0] = rng.uniform(-half, half, P).astype(F)
    g["means3D"][:, 1] = rng.uniform(-half, half, P).astype(F)
    g["means3D"][:, 2] = z
    g["means3D"][5::9, 2] = -1.0      # culled Gaussians (key 0xFFFFFFFF) do not count


def _small(i):
    rng = np.random.default_rng(7000 + i)
    V = int(rng.choice(VIEW_COUNTS, p=np.asarray(VIEW_WEIGHTS, np.float64) / sum(VIEW_WEIGHTS)))
    W, H = int(rng.choice(SIZES_W)), int(rng.choice(SIZES_H))
    P = int(rng.choice(POINTS))
    pin = PINNED.get(i, {})
    V, W, H, P = pin.get("V", V), pin.get("W", W), pin.get("H", H), pin.get("P", P)
    if V >= 31:                        # the few large batches get tiny clouds (and V = 256 images of at most 256 x 144)
        P = int(rng.choice(POINTS[:8]))
        if V == 256:
            W, H = min(W, 256), min(H, 144)
    D = int(rng.integers(0, 4))
    rows = int(rng.choice([(D + 1) ** 2, 16, 13 if D <= 2 else 16]))
    rows = max(rows, (D + 1) ** 2)
    scale = float(rng.choice(SCALES))
    spread = float(rng.choice([0.3, 1.0, 3.0]))
    fov = float(rng.choice(FOVS))
    aniso = float(rng.choice(ANISOTROPY))
    g = synth.random_scene(P, W, H, seed=8000 + i, sh_degree=D, sh_rows=rows, spread=spread, scale=scale, anisotropy=aniso)
    if rng.random() < 0.3:
        g["rotations"] = (g["rotations"] * rng.uniform(0.5, 1.6, (P, 1))).astype(F)       # kernels never normalise
    if rng.random() < 0.2:
        g["opacities"][:] = 1.0
    mode = "colors" if rng.random() < 0.25 else "sh"
    use_cov = bool(rng.random() < 0.25)
    mod = float(rng.choice([1.0, 1.0, 0.6, 2.5]))
    bg = tuple(float(x) for x in rng.uniform(0, 1, 3))
    slab = pin.get("slab", bool(rng.random() < 0.22))
    want_passes = None
    if slab:
        _slab(g, fov, rng)
        want_passes = [int(x) for x in rng.choice([1, 2, 3, 4], V)]
        want_passes[:min(V, 4)] = [int(x) for x in rng.permutation([1, 2, 3, 4])[:min(V, 4)]]    # odd and even counts in one batch
        views = []
        for k, n in enumerate(want_passes):
            axis, turn = int(rng.integers(0, 2)), float(rng.uniform(0.8, 1.25)) * float(rng.choice([-1.0, 1.0]))
            # (four passes: a grazing camera close to the slab; how close and how flat it has to be depends on the field of view,
            # so the first candidate that the host predicts to need four passes is taken)
            for theta, dist in [SLAB_VIEWS[n]] + ([(1.3, 0.9), (1.45, 1.3), (1.45, 1.0), (1.52, 1.3)] if n == 4 else []):
                view = _orbit(axis, theta * (turn if n != 4 else math.copysign(1.0, turn)), dist, W, H, fov)
                got = _predict_passes(dict(g=g, views=[view], fov=fov), 0)
                if got == n:
                    break
            if got is not None:
                want_passes[k] = got
            views.append(view)
    else:
        g["means3D"][:, 2] -= 3.0      # around the origin, where the circle cameras look
        if rng.random() < 0.15:
            g["means3D"][:, 2] -= 5.0
        circle = [_np_view(v) for v in camera.circle_views(n_imgs=12, fov_deg=fov, width_px=W, height_px=H)]
        views = []
        for _ in range(V):
            if rng.random() < 0.7:
                views.append(circle[int(rng.integers(0, 12))])
            else:                       # the identity camera three units back, tilted by up to 25 degrees and moved a little
                R = _rot(0, float(rng.uniform(-0.44, 0.44))) @ _rot(1, float(rng.uniform(-0.44, 0.44)))
                views.append(_camera(R, (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -3.0 + rng.uniform(-0.5, 0.5)), W, H, fov))
    empty = []
    if rng.random() < 0.3:
        where = {0: [0], 1: [V // 2], 2: [V - 1], 3: [0, V - 1], 4: [0, V // 2, V - 1]}[int(rng.integers(0, 5))]
        empty = sorted(set(where))
    if "empty" in pin:
        empty = pin["empty"]
    if empty:
        for v in empty:
            views[v] = _far(views[v])
            if want_passes is not None:
                want_passes[v] = 1      # no visible Gaussian: one pass, any order (sort.hip k_radix_rowscan)
    return dict(i=i, kind="small", g=g, views=views, W=W, H=H, bg=bg, mode=mode, scale_modifier=mod, use_cov3d=use_cov, fov=fov,
                slab=slab, want_passes=want_passes, empty=empty, params=dict(scale=scale, anisotropy=aniso, spread=spread, sh_degree=D))


def _medium(j):
    V, P, W, H = MEDIUM[j]
    rng = np.random.default_rng(9000 + j)
    cloud = synth.make_cloud("synth-THuman-800K", seed=j, P=P)
    g = synth.make_gaussians(cloud, profile="training", seed=1 + j)
    circle = [_np_view(v) for v in camera.circle_views(n_imgs=12, fov_deg=45.0, width_px=W, height_px=H)]
    pick = [int(x) for x in rng.permutation(12)]
    views = [circle[pick[v % 12]] for v in range(V)]
    empty = []
    if j % 3 == 1:                     # a view that sees nothing inside the ragged last row
        empty = [V - 1]
        views[V - 1] = _far(views[V - 1])
    return dict(i=MEDIUM_BASE + j, kind="medium", g=g, views=views, W=W, H=H, bg=(0.3, 0.3, 0.3), mode="sh", scale_modifier=1.0,
                use_cov3d=False, fov=45.0, slab=False, want_passes=None, empty=empty)


def case(i):
    return _medium(i - MEDIUM_BASE) if i >= MEDIUM_BASE else _small(i)


def scenes(c):
    """one oracle Scene per view"""
    return [util.scene_from(c["g"], v, c["W"], c["H"], bg=c["bg"], mode=c["mode"], scale_modifier=c["scale_modifier"],
                            use_cov3d=c["use_cov3d"]) for v in c["views"]]


def dL_dpix(c):
    """the seeded image gradients of a case, [V, 3, H, W]"""
    i = c["i"]
    return np.random.default_rng(77 + i).uniform(-1, 1, (len(c["views"]), 3, c["H"], c["W"])).astype(F)


def fingerprint(c):
    h = hashlib.sha256()
    for k in sorted(c["g"]):
        h.update(k.encode())
        h.update(np.ascontiguousarray(c["g"][k]).tobytes())
    for v in c["views"]:
        for k in ("viewmatrix", "projmatrix", "campos"):
            h.update(v[k].tobytes())
        h.update(repr((v["tanfovx"], v["tanfovy"])).encode())
    h.update(repr((c["W"], c["H"], c["bg"], c["mode"], c["scale_modifier"], c["use_cov3d"], c["empty"], c["want_passes"])).encode())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------ the launch formulas
def _div_up(a, b):
    return (a + b - 1) // b


def preprocess_vpt(V, P):
    """preprocess.hip launch_preprocess: (views per thread, grid rows, views of the last row)"""
    blocks = _div_up(P, 256)
    vpt = 1
    while vpt < V and blocks * _div_up(V, vpt * 2) >= 2048:
        vpt *= 2
    vpt = min(vpt, V)
    rows = _div_up(V, vpt)
    return vpt, rows, V - (rows - 1) * vpt


def tile_sort_passes(T):
    """host.hpp tile_bits / sort.hip: ceil(bit_length(T) / 8) passes over the pairs"""
    return _div_up(int(T).bit_length(), 8)


def backward_dynamic(V, T):
    """render_bwd.hip launch_render_backward: pulled work units when the static grid would exceed 4096 groups of 32 workgroups"""
    return V > 1 and _div_up(T, 8) * V > 4096


def slice_length(V):
    """common.hpp bwd_chunk_shift: list entries per backward work item"""
    return 1024 if V >= 2 else 512


def depth_sort_words(keys):
    """sort.hip k_radix_rowscan: (base, bits, passes) from the depth keys (uint32) of the Gaussians that emit pairs"""
    keys = np.asarray(keys, np.uint32)
    if keys.size == 0:
        return 0, 8, 1
    base = int(keys.min()) & ~0xFF
    span = int(keys.max()) - base
    bits = max(8, span.bit_length())
    return base, bits, _div_up(bits, 8)


def _predict_passes(c, v):
    """Depth-sort passes of view v of a slab case, or None where the host cannot tell.  The pass count grows with the interval of
    the keys of the Gaussians that emit pairs: those whose centre projects well inside the image certainly do, those in front of
    the near plane may; the prediction stands where both intervals (the first narrowed, the second widened by 64 codes against
    float32 rounding of the view transform) give the same count."""
    view = c["views"][v]
    m = c["g"]["means3D"].astype(np.float64)
    vm = view["viewmatrix"].astype(np.float64).reshape(4, 4)
    pv = m @ vm[:3, :3] + vm[3, :3]
    z = pv[:, 2]
    t = math.tan(math.radians(c["fov"]) / 2)
    front = z > 0.2
    if not front.any():
        return 1
    inside = (z > 0.25) & (np.abs(pv[:, 0]) < 0.9 * t * z) & (np.abs(pv[:, 1]) < 0.9 * t * z)
    if not inside.any():
        return None
    ki = z[inside].astype(F).view(np.uint32).astype(np.int64)
    ko = z[front].astype(F).view(np.uint32).astype(np.int64)
    # (a camera whose axis is the world's z axis computes view-space z = z + t without rounding: no margin needed)
    mg = 0 if np.array_equal(vm[:3, 2], [0.0, 0.0, 1.0]) and vm[3, 2] == 0.0 else 64
    lo = depth_sort_words(np.array([ki.min() + mg, max(ki.max() - mg, ki.min() + mg)], np.int64).astype(np.uint32))[2]
    hi = depth_sort_words(np.array([max(ko.min() - mg, 0), ko.max() + mg], np.int64).astype(np.uint32))[2]
    return lo if lo == hi else None


def expected(i, c=None):
    """the branches case i takes, from the launch formulas"""
    c = case(i) if c is None else c
    V, P, W, H = len(c["views"]), c["g"]["means3D"].shape[0], c["W"], c["H"]
    T = _div_up(W, 16) * _div_up(H, 16)
    vpt, rows, last = preprocess_vpt(V, P)
    passes = None
    if c["slab"]:
        passes = [1 if v in c["empty"] else _predict_passes(c, v) for v in range(V)]
    known = sorted(set(p for p in (passes or []) if p is not None))
    return dict(V=V, P=P, W=W, H=H, T=T, vpt=vpt, grid_rows=rows, last_row_views=last, ragged=last != vpt,
                dynamic=backward_dynamic(V, T), tile_sort_passes=tile_sort_passes(T), slice_length=slice_length(V),
                empty=list(c["empty"]), depth_passes=passes,
                mixed=len(known) >= 2 and any(p & 1 for p in known) and any(not p & 1 for p in known))
