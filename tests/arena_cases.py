"""Pairs of frames for the arena contract (tests/test_gpu_arena_state.py): a call's results must not depend on what the caller's
arenas held before it.  Importable without torch, the built library or a device.

A pair is a donor D and a subject S that share P, W, H, tan-fov and the width of the SH table, so that the geometry, image, binning
and extra-state arenas carve identically; they differ in cloud, cameras, colours and active SH degree.  D's calls leave the arenas
in a valid state of ANOTHER frame, S's calls run on top of it, and everything S returns must carry the bits of the same calls on
zero-filled arenas.

  PAIRS / pair(name)        main (three views, S's last one sees nothing), culled (S sees nothing anywhere), pingpong (depth sorts
                            that end in different buffers), deep (lists longer than a backward slice, in different tiles)
  scenes(pair, who, V)      the oracle Scenes of D ("D") or S ("S"), the first V views
  dL_dpix / channel_values  seeded image gradients and extra-channel inputs of a pair
  census(pair, oracle)      what the oracle's forwards of D and S say about the pair, view by view: which tiles empty out, how long
                            the lists are, who is visible, where the SH clamp masks differ, how many passes the depth sorts run,
                            which pixel quadrants walk past a slice boundary -- the facts tests/test_cpu_arena_cases.py holds the
                            scene parameters to, from the oracle alone
  CASES                     the names of the GPU cases
  outputs / differing       the compared arrays of one run under their names; the names whose bits differ between two runs

The cameras and slabs are batch_cases' own (BC._orbit, BC._far, BC._slab: its generator's pieces, underscore and all): the slab views'
pass counts are what that module already predicts and pins, and a second copy of them here would drift."""
import math

import numpy as np

import batch_cases as BC
import util
from pcrender import synth

F = np.float32
P = 2900                  # 11 workgroups of 256 and a ragged one of 84; 45 waves and 20 lanes
FOV = 50.0
SH_ROWS = 16
PAIRS = ("main", "culled", "pingpong", "deep")
SLICES = (512, 1024)      # common.hpp bwd_chunk_shift: list entries per backward slice at V = 1 / from V = 2
# the cases of tests/test_gpu_arena_state.py, each named after the invariant it holds (DESIGN.md section 6 refers to them by name)
CASES = {
    "frame_after_backward": "a training frame and its followers on arenas a donor's forward and atomic backward used",
    "records_after_inference_frame": "dirty gradient records under a fast-arithmetic inference frame that cleared nothing",
    "inference_after_training_frame": "an inference frame and its contribution statistics on a training frame's arenas",
    "view_count_change": "another number of views on the same allocations: other strides, another slice length",
    "recolor_rewrites_saves": "backwards after need_backward recolors, shared colours and colours per view",
    "channels_state": "channels frames of another width, and colour frames, on each other's arenas and extra-state block",
    "resume_on_used_binning": "a retried frame resumed on a binning arena a donor filled",
    "stage_pair": "the count-then-bind pair on a donor's arenas",
    "nothing_visible": "a view or a whole batch in which every Gaussian is culled, after a full donor",
    "depth_sort_ping_pong": "depth sorts that end in the other ping-pong buffer than the donor's",
}


def _cloud(W, H, seed, sh_degree, u, v, z, scale, opacity=None, parts=None):
    """synth.random_scene's Gaussians with the centres placed by screen position for the identity camera: normalised device
    coordinates u, v (ranges; the image is [-1, 1] both ways) at depth z (range).  parts: [(count, u range, v range)] instead of one
    range for all"""
    g = synth.random_scene(P, W, H, seed=seed, sh_degree=sh_degree, sh_rows=SH_ROWS, scale=scale)
    rng = np.random.default_rng(seed + 500)
    th = math.tan(math.radians(FOV) / 2)
    parts = [(P, u, v)] if parts is None else parts
    assert sum(n for n, _, _ in parts) == P
    uu = np.concatenate([rng.uniform(a[0], a[1], n) for n, a, _ in parts])
    vv = np.concatenate([rng.uniform(b[0], b[1], n) for n, _, b in parts])
    zz = rng.uniform(z[0], z[1], P)
    g["means3D"] = np.stack([uu * th * zz, vv * th * zz, zz], 1).astype(F)
    if opacity is not None:
        g["opacities"] = rng.uniform(opacity[0], opacity[1], (P, 1)).astype(F)
    return g


def _views(W, H, turns):
    """cameras two units from the pivot (0, 0, 2), turned by (axis, angle); angle 0 is the identity camera"""
    return [BC._orbit(axis, theta, 2.0, W, H, FOV) for axis, theta in turns]


def pair(name):
    """dict(name, W, H, V, D = (Gaussians, views, bg), S = likewise)"""
    if name in ("main", "culled"):
        # D fills the left five of the seven tile columns, S the right three at a lower SH degree; part of S's cloud lies behind
        # the cameras
        W, H = 112, 96
        gd = _cloud(W, H, 101, 2, (-0.95, 0.36), (-0.95, 0.95), (1.6, 2.4), 0.035)
        gs = _cloud(W, H, 202, 1, (0.32, 0.95), (-0.6, 0.9), (1.7, 2.3), 0.012)
        gs["means3D"][::7, 2] = -1.0
        vd = _views(W, H, [(0, 0.0), (1, 0.06), (0, -0.08)])
        vs = _views(W, H, [(1, 0.03), (0, 0.05), (1, -0.04)])
        vs[2] = BC._far(vs[2])
        if name == "culled":
            vs = [BC._far(x) for x in vs]
        return dict(name=name, W=W, H=H, V=3, D=(gd, vd, (0.2, 0.4, 0.6)), S=(gs, vs, (0.7, 0.1, 0.3)))
    if name == "pingpong":
        # BC's slabs: depth keys within 200 codes for the identity camera; the turn of a camera sets the number of key bits that
        # differ, and with it the passes of the depth sort (1, 2, 3 for D; 2, 3, 4 for S: another parity in every view)
        W, H = 112, 96
        gd = synth.random_scene(P, W, H, seed=303, sh_degree=2, sh_rows=SH_ROWS, scale=0.03)
        gs = synth.random_scene(P, W, H, seed=404, sh_degree=1, sh_rows=SH_ROWS, scale=0.015)
        BC._slab(gd, FOV, np.random.default_rng(31))
        BC._slab(gs, FOV, np.random.default_rng(41))
        gs["means3D"][:, 0] *= F(0.5)
        gs["means3D"][3::9, 2] = -1.0          # (another ninth of S behind the cameras: Gaussians that only D sees)
        vd = [BC._orbit(1, BC.SLAB_VIEWS[n][0], BC.SLAB_VIEWS[n][1], W, H, FOV) for n in (1, 2, 3)]
        vs = [BC._orbit(0, BC.SLAB_VIEWS[n][0], BC.SLAB_VIEWS[n][1], W, H, FOV) for n in (2, 3, 4)]
        return dict(name=name, W=W, H=H, V=3, D=(gd, vd, (0.0, 0.0, 0.0)), S=(gs, vs, (1.0, 1.0, 1.0)))
    if name == "deep":
        # util.build_scene("deep_stack") cut down: five tiles in a row, faint splats that no pixel terminates on.  D stacks 2300 of
        # them in the first tile, 300 in the second and 150 in each of the last two, which S leaves empty; S stacks 2600 in the
        # second tile (its widest reach into the third) and 300 in the first, half of those behind the cameras: each has a list longer than 1024 entries where the
        # other's is shorter than 512
        W, H = 80, 16
        col, rows = [(-0.85 + 0.4 * k, -0.75 + 0.4 * k) for k in range(5)], (-0.5, 0.5)
        gd = _cloud(W, H, 505, 1, None, None, (1.0, 3.0), 0.05, opacity=(0.008, 0.015),
                    parts=[(2300, col[0], rows), (300, col[1], rows), (150, col[3], rows), (150, col[4], rows)])
        gs = _cloud(W, H, 606, 2, None, None, (1.0, 3.0), 0.05, opacity=(0.008, 0.015), parts=[(300, col[0], rows), (2600, col[1], rows)])
        gs["means3D"][:150, 2] = -1.0          # (behind the cameras: visible in D only, and S's lists are shorter than D's)
        for g in (gd, gs):
            g["rotations"] = np.tile(np.array([1, 0, 0, 0], F), (P, 1))
        vd = _views(W, H, [(0, 0.0), (1, 0.004), (0, -0.004)])
        vs = _views(W, H, [(0, 0.002), (1, -0.003), (0, 0.005)])
        return dict(name=name, W=W, H=H, V=3, D=(gd, vd, (0.2, 0.3, 0.4)), S=(gs, vs, (0.5, 0.1, 0.9)))
    raise KeyError(name)


def scenes(pr, who, V=None):
    """the oracle Scenes of the pair's donor ("D") or subject ("S"): one per view, the first V of them"""
    g, views, bg = pr[who]
    return [util.scene_from(g, v, pr["W"], pr["H"], bg=bg) for v in views[:pr["V"] if V is None else V]]


def dL_dpix(pr, who, V=None):
    V = pr["V"] if V is None else V
    seed = (PAIRS.index(pr["name"]) + 1) * 10 + (who == "S")
    return np.random.default_rng(seed).uniform(-1, 1, (V, 3, pr["H"], pr["W"])).astype(F)


def channel_values(pr, who, nx, V=None):
    """the inputs of a channels call: (values -- nx = 8: the split pair ([P,4], [V,P,4]); nx = 4: [P,4] --, view scales [V,nx],
    bg_extra [nx], dL_dextra [V,nx,H,W])"""
    V = pr["V"] if V is None else V
    rng = np.random.default_rng(900 + nx + (who == "S"))
    x = (rng.normal(0, 1, (P, 4)).astype(F), rng.normal(0, 1, (V, P, 4)).astype(F)) if nx == 8 else rng.normal(0, 1, (P, 4)).astype(F)
    return (x, rng.choice(np.array([-2.0, -0.5, 0.5, 3.0], F), (V, nx)).astype(F), rng.uniform(-1, 1, nx).astype(F),
            rng.uniform(-1, 1, (V, nx, pr["H"], pr["W"])).astype(F))


# ---- what the oracle says about a pair ------------------------------------------------------------------------------------------
def _crossing(fw, L):
    """the 8 x 8 pixel quadrants of a forward whose walk certainly passes list position L of their tile: some pixel's last
    contributor lies behind it; as a set of (tile, quadrant)"""
    H, W, gx = fw["H"], fw["W"], fw["gridx"]
    out = set()
    ys, xs = np.nonzero(fw["n_contrib"].reshape(H, W) > L)
    for y, x in zip(ys, xs):
        out.add(((y // 16) * gx + x // 16, ((y % 16) // 8) * 2 + (x % 16) // 8))
    return out


def _short(fw, L):
    """the quadrants of tiles whose whole list is at most L entries long: they cannot pass position L"""
    n = fw["ranges"].astype(np.int64)
    return {(int(t), q) for t in np.nonzero(n[:, 1] - n[:, 0] <= L)[0] for q in range(4)}


def census(pr, oracle):
    """The facts about a pair, from the oracle's forwards of D and S view by view (a list of dicts, one per view):
      tiles, d_only, s_only      tiles of the image; tiles with a list in D and none in S; the other way round
      pairs_d, pairs_s           num_rendered
      longest_d, longest_s       the longest tile list
      visible_d_only             Gaussians (by index) visible in D and invisible in S; both: visible in both
      clamp_differs              ... of those, the ones whose SH clamp masks differ
      passes_d, passes_s         passes of the depth sort (BC.depth_sort_words of the visible Gaussians' depth keys)
      cross_d_only, cross_s_only {slice length: quadrants whose walk passes the first slice boundary in D and cannot in S; vice versa}"""
    out = []
    for sd, ss in zip(scenes(pr, "D"), scenes(pr, "S")):
        d, s = oracle.forward(sd), oracle.forward(ss)
        ld = d["ranges"].astype(np.int64)[:, 1] - d["ranges"].astype(np.int64)[:, 0]
        ls = s["ranges"].astype(np.int64)[:, 1] - s["ranges"].astype(np.int64)[:, 0]
        vd, vs = d["radii"] > 0, s["radii"] > 0
        both = vd & vs
        out.append(dict(
            tiles=int(ld.size), d_only=int(((ld > 0) & (ls == 0)).sum()), s_only=int(((ld == 0) & (ls > 0)).sum()),
            pairs_d=int(d["R"]), pairs_s=int(s["R"]), longest_d=int(ld.max()), longest_s=int(ls.max()),
            visible_d=int(vd.sum()), visible_s=int(vs.sum()), visible_d_only=int((vd & ~vs).sum()), both=int(both.sum()),
            clamp_differs=int((d["clamped"][both] != s["clamped"][both]).any(1).sum()),
            passes_d=BC.depth_sort_words(d["depths"][vd].view(np.uint32))[2],
            passes_s=BC.depth_sort_words(s["depths"][vs].view(np.uint32))[2],
            cross_d_only={L: len(_crossing(d, L) & _short(s, L)) for L in SLICES},
            cross_s_only={L: len(_crossing(s, L) & _short(d, L)) for L in SLICES}))
    return out


# ---- comparing two runs ---------------------------------------------------------------------------------------------------------
def outputs(**arrays):
    """the compared arrays of one run under their names: numpy arrays as they are, lists and tuples of arrays as name[i], scalars as
    0-d arrays; None is left out"""
    out = {}
    for k, a in arrays.items():
        if a is None:
            continue
        if isinstance(a, (list, tuple)) and any(isinstance(x, np.ndarray) for x in a):
            for i, x in enumerate(a):
                out["%s[%d]" % (k, i)] = np.ascontiguousarray(x)
        else:
            out[k] = np.ascontiguousarray(a)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize in (4, 8) and a.dtype.kind in "fiu":
        return a.reshape(-1).view(np.uint32)
    return a.reshape(-1).view(np.uint8)


def differing(a, b):
    """the names whose bits differ between two outputs() dicts, sorted: a name only one of them has, another shape or dtype, or
    another bit anywhere.  Floats are compared as uint32 words: equal NaN payloads are equal, +0 and -0 are not"""
    bad = set(a) ^ set(b)
    for k in set(a) & set(b):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(_bits(x), _bits(y)):
            bad.add(k)
    return sorted(bad)
