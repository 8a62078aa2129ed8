"""The seeded scenes of the camera-gradient tests (tests/test_gpu_camera_backward.py, tests/test_cpu_camera_cases.py), their float64
reference -- the oracle's float64 render backward feeding tests/fp64_camera.py, computed once per case -- and the bar a library
result is held to."""
import functools

import numpy as np

import util
from fp64_camera import DEAD_PROJ, DEAD_VIEW, LIVE_PROJ, LIVE_VIEW, camera_backward_fp64

CAM_ROWS = 1024          # Gaussians per workgroup of k_camera_partials: CAM_ROWS of csrc/common.hpp
CAM_SUM_THREADS = 256    # threads of k_camera_sum (one workgroup per view): CAM_THREADS of csrc/common.hpp
EDGE_SIZES = (CAM_ROWS - 1, CAM_ROWS, CAM_ROWS + 1, 2 * CAM_ROWS + 3)
MANY_PARTIALS_P = CAM_ROWS * (CAM_SUM_THREADS + 1) + 5   # k_camera_sum's per-thread loop runs twice for two threads, once for the rest

# (name, live entries, entries the forward never reads)
TENSORS = (("dL_dviewmatrix", LIVE_VIEW, DEAD_VIEW), ("dL_dprojmatrix", LIVE_PROJ, DEAD_PROJ), ("dL_dcampos", [0, 1, 2], []))
N_LIVE = sum(len(t[1]) for t in TENSORS)


def pose(seed):
    """H_c2w of a camera a little off the origin and a little rotated, looking down +z: every live matrix entry has a value of its own"""
    import torch
    rng = np.random.default_rng(seed)
    w = rng.uniform(-0.15, 0.15, 3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    H = np.eye(4)
    H[:3, :3] = np.eye(3) + K + K @ K / 2          # (nearly a rotation; inv_homogeneous treats it as one, the map is smooth either way)
    H[:3, 3] = rng.uniform(-0.2, 0.2, 3)
    return torch.as_tensor(H, dtype=torch.float32)


def looking_away():
    """a camera at z = -5 turned half a turn about y: the whole cloud (depths -1 .. 4) is behind it"""
    import torch
    H = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0]))
    H[2, 3] = -5.0
    return H


def cloud(P, seed, degree, xy=0.8, scale=(0.3, 0.6)):
    """P Gaussians in front of pose(): depths 2..4, footprints of a pixel and more on a 70 x 50 image, no needles"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 4.0, P)
    means = np.stack([rng.uniform(-xy, xy, P) * z / 3, rng.uniform(-xy, xy, P) * z / 3, z], 1).astype(np.float32)
    shs = (0.15 * rng.standard_normal((P, 16, 3))).astype(np.float32)
    shs[:, 0, :] = rng.normal(0.3, 1.2, (P, 3))
    q = rng.standard_normal((P, 4))
    return dict(means3D=means, scales=rng.uniform(scale[0], scale[1], (P, 3)).astype(np.float32),
                rotations=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                opacities=rng.uniform(0.1, 0.6, (P, 1)).astype(np.float32), shs=shs, sh_degree=degree,
                colors_precomp=rng.uniform(0.0, 1.0, (P, 3)).astype(np.float32))


def mixed_cloud(degree=3, seed=11, P=300):
    """a cloud with Gaussians outside the frustum clamp, behind the camera and with clamped colour channels"""
    g = cloud(P, seed, degree, scale=(0.1, 0.4))
    # x / z (y / z) beyond 1.3 tanfov -- tanfov is the tangent of the FULL angle, the image ends at the half angle's -- and large enough
    # to reach the image from there (a splat whose tile rectangle is empty is culled)
    g["means3D"][::17, 0] = 2.4 * g["means3D"][::17, 2]
    g["means3D"][3::23, 1] = -2.4 * g["means3D"][3::23, 2]
    g["scales"][::17] = 5.0
    g["scales"][3::23] = 5.0
    g["means3D"][5::13, 2] = -1.0                             # behind the camera
    return g


def views_of(g, poses, W, H, **kw):
    return [util.scene_from(g, util._view_arrays(Hc, W, H, 60.0), W, H, **kw) for Hc in poses]


def mixed_scene(degree=3, W=70, H=50):
    return views_of(mixed_cloud(degree), [pose(3)], W, H)[0]


def build(name):
    """(scenes -- one per view --, dL_dpix per view) of a named case"""
    if name == "one":
        g = dict(means3D=np.array([[0.1, -0.05, 2.5]], np.float32), scales=np.array([[0.5, 0.2, 0.3]], np.float32),
                 rotations=np.array([[0.9, 0.1, 0.3, -0.2]], np.float32), opacities=np.array([[0.8]], np.float32),
                 shs=np.array([[[0.5, -0.2, 0.1], [0.3, 0.1, -0.2], [-0.1, 0.2, 0.3], [0.2, -0.3, 0.1]]], np.float32), sh_degree=1)
        scenes = views_of(g, [pose(1)], 16, 16)
    elif name.startswith("edges_"):
        scenes = views_of(cloud(int(name[6:]), 21, 2, scale=(0.1, 0.3)), [pose(3), pose(4), pose(5)], 70, 50, bg=(0.2, 0.3, 0.4))
    elif name in ("mixed_sh0", "mixed_sh3"):
        scenes = views_of(mixed_cloud(int(name[-1])), [pose(3), looking_away(), pose(4)], 70, 50)
    elif name == "mixed_precomp":
        scenes = views_of(mixed_cloud(0), [pose(3), looking_away(), pose(4)], 70, 50, mode="colors", use_cov3d=True)
    elif name == "channels":
        scenes = views_of(cloud(700, 31, 1, scale=(0.1, 0.3)), [pose(3), pose(6)], 70, 50)
    else:
        raise KeyError(name)
    return scenes, [util.seeded_dL(s, seed=123 + v) for v, s in enumerate(scenes)]


ARBITER_CASES = ("one",) + tuple("edges_%d" % n for n in EDGE_SIZES) + ("mixed_sh0", "mixed_sh3", "mixed_precomp")


def channels_inputs(scenes, nx=4, seed=77):
    """(values [P,nx] shared by the views, view scales [V,nx], bg_extra [nx], dL_dextra [V,nx,H,W]) of the channels case"""
    rng = np.random.default_rng(seed)
    s, V = scenes[0], len(scenes)
    return (rng.normal(0, 1, (s.P, nx)).astype(np.float32), rng.choice(np.array([-2.0, 0.5, 1.0, 3.0], np.float32), (V, nx)),
            rng.uniform(-1, 1, nx).astype(np.float32), rng.uniform(-1, 1, (V, nx, s.H, s.W)).astype(np.float32))


def _per_view(scenes, views, sums32):
    exact = [camera_backward_fp64(s, w["fwd"]["radii"], w["fwd"]["clamped"], w["exact"]["dL_dmean2D"], w["exact"]["dL_dconic"],
                                  w["exact"]["dL_dcolor"]) for s, w in zip(scenes, views)]
    yard = [camera_backward_fp64(s, w["fwd"]["radii"], w["fwd"]["clamped"], w[sums32]["dL_dmean2D"], w[sums32]["dL_dconic"],
                                 w[sums32]["dL_dcolor"], dtype=np.float32) for s, w in zip(scenes, views)]
    return exact, yard


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(scenes, dLs, f64 = the grad_ladder.Float64 of the case, exact / yard = per view the arbiter's result in float64 from the
    float64 render-level sums / in float32 from the plain-C oracle's float32 sums).  Computed once, shared by the tests, not modified."""
    from grad_ladder import ChannelsFloat64, Float64
    scenes, dLs = build(name)
    if name == "channels":
        x, sc, bgx, dx = channels_inputs(scenes)
        f64 = ChannelsFloat64(scenes, np.ascontiguousarray(np.broadcast_to(x, (len(scenes),) + x.shape)), sc, bgx, np.stack(dLs), dx)
        exact, yard = _per_view(scenes, f64.views(), "f32")
    else:
        f64 = Float64(scenes, dLs)
        exact, yard = _per_view(scenes, f64.views(), "grads32")
    return dict(scenes=scenes, dLs=dLs, f64=f64, exact=exact, yard=yard)


def hold(lib, exact, yard, tag):
    """One view's library result (dict of the three arrays) against the arbiter: per tensor, with e = |lib - exact|,
    plain = util.GRAD_ABS * max|exact| and y = |yardstick - exact|, every live entry needs e <= max(plain, 4 y); every output is finite
    and the dead entries are exactly +0.  Returns (live entries that needed the 4 y exit, worst e / plain)."""
    exits, worst = 0, 0.0
    for name, live, dead in TENSORS:
        a = np.asarray(lib[name], np.float32).reshape(-1)
        assert np.isfinite(a).all(), "%s %s: non-finite" % (tag, name)
        assert (a[dead].view(np.uint32) == 0).all(), "%s %s: a dead entry is not +0" % (tag, name)
        x = np.asarray(exact[name], np.float64).reshape(-1)[live]
        y = np.abs(np.asarray(yard[name], np.float64).reshape(-1)[live] - x)
        e = np.abs(a.astype(np.float64)[live] - x)
        if np.abs(x).max() == 0:
            assert (a.view(np.uint32) == 0).all(), "%s %s: exact is zero, the library's is not +0" % (tag, name)
            continue
        plain = util.GRAD_ABS * np.abs(x).max()
        assert (e <= np.maximum(plain, 4 * y)).all(), "%s %s: |lib - exact| up to %.3g, plain bar %.3g, 4 x yardstick up to %.3g" % (
            tag, name, e.max(), plain, (4 * y).max())
        exits += int((e > plain).sum())
        worst = max(worst, float(e.max() / plain))
    return exits, worst


def census(s, fwd):
    """(frustum-clamped and visible, invisible, visible with a clamped colour channel) index sets of a scene and its forward state"""
    V = s.viewmatrix.astype(np.float64)
    t = s.means3D.astype(np.float64) @ np.array([[V[0], V[4], V[8]], [V[1], V[5], V[9]], [V[2], V[6], V[10]]]).T + V[12:15]
    vis = fwd["radii"] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (np.abs(t[:, 0] / t[:, 2]) > np.float32(1.3) * np.float32(s.tanfovx)) | (np.abs(t[:, 1] / t[:, 2]) > np.float32(1.3) * np.float32(s.tanfovy))
    col = np.asarray(fwd["clamped"], bool).any(1) if s.shs is not None else np.zeros(s.P, bool)
    return np.nonzero(out & vis)[0], np.nonzero(~vis)[0], np.nonzero(col & vis)[0]


def translation_identity(scenes, gm, cams):
    """(left, right) of  sum_i dL_dmean3D[i][j] = sum_v (sum_k view[k+4j] dV[12+k] + sum_{k in 0,1,3} proj[k+4j] dP[12+k] - dC[j]):
    gm [P,3] the mean gradient summed over the views, cams the per-view camera gradients"""
    right = np.zeros(3)
    for s, cg in zip(scenes, cams):
        V, Pm = s.viewmatrix.astype(np.float64), s.projmatrix.astype(np.float64)
        dV, dP, dC = (np.asarray(cg[n], np.float64).reshape(-1) for n in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"))
        right += np.array([sum(V[k + 4 * j] * dV[12 + k] for k in range(3)) + sum(Pm[k + 4 * j] * dP[12 + k] for k in (0, 1, 3)) - dC[j]
                           for j in range(3)])
    return np.asarray(gm, np.float64).sum(0), right
