"""What the randomised sweeps, the deterministic-backward tests and the full-size tests share.  Importable without torch, the built
library or a device.  The tallies the sweeps fill stay in their test modules and are passed in.

  random_case / check_random_case            the single-view sweep: case i, and its comparison against the reference build
  records_backward / nine_tensors_backward   one colour backward on a run's arenas: (gradients, records) / one dict of nine arrays
  same_bits                                  two dicts of float32 arrays, bit for bit
  check_view_against_reference               one view of a batch forward against the reference build's forward of that view
  uniform_dpix / power_scene / leaves        the deterministic tests' seeded dL_dpix, non-repeatable scene and autograd leaves
  FULLSIZE_CONFIGS / fullsize_scene          the benchmark's full-size configurations
  fd_single_gaussians                        central differences of the forward, one Gaussian at a time"""
import numpy as np

import batch_cases as BC
import native_calls as NC
import util
from grad_ladder import Float64, hold_to_reference

F = np.float32


# ---- the single-view sweep --------------------------------------------------------------------------------------------------------
def random_case(i):
    from pcrender import camera, synth
    rng = np.random.default_rng(1000 + i)
    W = int(rng.choice([1, 7, 16, 17, 31, 33, 64, 97, 130, 200]))
    H = int(rng.choice([1, 5, 16, 23, 32, 48, 65, 111]))
    P = int(rng.choice([1, 2, 63, 64, 65, 300, 1500, 4000]))
    D = int(rng.integers(0, 4))
    rows = int(rng.choice([(D + 1) ** 2, 16, 13 if D <= 2 else 16]))
    rows = max(rows, (D + 1) ** 2)
    scale = float(rng.choice([0.004, 0.02, 0.05, 0.15, 0.4]))
    spread = float(rng.choice([0.3, 1.0, 3.0]))
    g = synth.random_scene(P, W, H, seed=2000 + i, sh_degree=D, sh_rows=rows, spread=spread, scale=scale,
                           anisotropy=float(rng.choice([0.5, 1.0, 2.0])))
    if rng.random() < 0.3:
        g["rotations"] = (g["rotations"] * rng.uniform(0.5, 1.6, (P, 1))).astype(np.float32)   # kernels never normalise (Q3)
    if rng.random() < 0.2:
        g["opacities"][:] = 1.0
    if rng.random() < 0.15:
        g["means3D"][:, 2] -= 5.0                                                              # mostly behind the camera
    mode = "colors" if rng.random() < 0.25 else "sh"
    use_cov = bool(rng.random() < 0.25)
    mod = float(rng.choice([1.0, 1.0, 0.6, 2.5]))
    bg = tuple(float(x) for x in rng.uniform(0, 1, 3))
    if rng.random() < 0.5:
        view = util.identity_camera(W, H, float(rng.choice([30.0, 45.0, 60.0, 80.0])))
    else:                                   # the reference caller's circle camera, looking at the origin from r = 3
        view = camera.circle_views(n_imgs=12, fov_deg=45.0, width_px=W, height_px=H)[int(rng.integers(0, 12))]
        g["means3D"][:, 2] -= 3.0
    return util.scene_from(g, view, W, H, bg=bg, mode=mode, scale_modifier=mod, use_cov3d=use_cov), mode


def check_random_case(i, dev, tally):
    """case i rendered by the library and by the reference build: integer outputs and forward floats bit for bit, gradients through
    the counted ladder of tests/grad_ladder.py"""
    ref = util.reference_build("strict")
    s, mode = random_case(i)
    dL = util.seeded_dL(s, seed=77 + i)
    r, gr = ref.forward_backward(s, dL)
    p, gp = util.run_product(s, dev, dL_dpix=dL)
    assert p["R"] == r["R"]
    for k in ("radii", "tiles_touched", "vals", "keys", "ranges", "n_contrib"):
        np.testing.assert_array_equal(p[k], r[k], err_msg="case %d %s" % (i, k))
    vis = r["radii"] > 0
    for k in ("depths", "means2D", "conic_opacity") + (() if mode == "colors" else ("rgb",)):
        assert p[k][vis].tobytes() == r[k][vis].tobytes(), "case %d %s" % (i, k)
    assert p["final_T"].tobytes() == r["final_T"].tobytes()
    assert p["out_color"].tobytes() == r["out_color"].tobytes()
    # the gradient comparison and its counted fallbacks: tests/grad_ladder.py (shared with the batched sweep)
    hold_to_reference("case %d" % i, 4242 + i, gp, gr, Float64([s], [dL]), tally)


# ---- a backward on a run's arenas -------------------------------------------------------------------------------------------------
def records_backward(N, args, run, dL_t, det, pairs=None):
    """one colour backward on the arenas of `run`: the eight gradients and the per-view records [V, P, 16], numpy"""
    g = N.rasterize_gaussians_backward_batch(*NC.colour_backward_args(args, run, dL_t), deterministic=det, pairs=pairs)
    out = {n: t.detach().cpu().numpy() for n, t in zip(util.GRAD_NAMES, g)}
    P, V = args[1].shape[0], dL_t.shape[0]
    rec = np.stack([N.grad_records(run[3], P, view=v, n_views=V).cpu().numpy() for v in range(V)])
    return out, rec


def nine_tensors_backward(N, args, run, dpix, det, dev):
    """one colour backward on the arenas of `run`: the eight per-Gaussian gradients and the per-view records (which hold dL_dconic),
    as numpy arrays: nine tensors"""
    out, rec = records_backward(N, args, run, NC.to_device(dpix, dev), det)
    out["records"] = rec
    return out


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def view_query(N, name, P, W, H, R, run, v, V):
    return N.query(name, P, W, H, R, run[3], run[4], run[5], view=v, n_views=V)


def check_view_against_reference(N, tag, r, run, v, V, P, W, H, mode):
    counts, color, radii = run[:3]
    assert counts[v] == r["R"], tag
    np.testing.assert_array_equal(radii[v].cpu().numpy(), r["radii"], err_msg=tag + " radii")
    R = r["R"]
    for name, key, dt in (("TILES_TOUCHED", "tiles_touched", np.uint32), ("POINT_LIST", "vals", np.uint32),
                          ("POINT_LIST_KEYS", "keys", np.uint64), ("RANGES", "ranges", np.uint32), ("N_CONTRIB", "n_contrib", np.uint32)):
        a = view_query(N, name, P, W, H, R, run, v, V).cpu().numpy().view(dt)
        np.testing.assert_array_equal(a.reshape(-1), np.asarray(r[key]).astype(dt).reshape(-1), err_msg="%s %s" % (tag, key))
    vis = r["radii"] > 0
    for name, key in (("DEPTHS", "depths"), ("MEANS2D", "means2D"), ("CONIC_OPACITY", "conic_opacity")) + \
            (() if mode == "colors" else (("RGB", "rgb"),)):
        a = view_query(N, name, P, W, H, R, run, v, V).cpu().numpy()
        assert a[vis].tobytes() == r[key][vis].tobytes(), "%s %s" % (tag, key)
    assert view_query(N, "FINAL_T", P, W, H, R, run, v, V).cpu().numpy().tobytes() == r["final_T"].tobytes(), tag + " final_T"
    assert color[v].cpu().numpy().tobytes() == r["out_color"].tobytes(), tag + " out_color"
    # the view's depth-sort control words: what sort.hip derives from the keys (depth bits) of the Gaussians that emit pairs
    words = view_query(N, "DEPTH_SORT", P, W, H, R, run, v, V).cpu().numpy().view(np.uint32)
    want = BC.depth_sort_words(r["depths"][vis].view(np.uint32))
    assert tuple(int(x) for x in words[:3]) == want, "%s depth-sort control words %s, the view's keys imply %s" % (tag, words[:3], want)
    return int(words[2])


# ---- the deterministic tests ------------------------------------------------------------------------------------------------------
def uniform_dpix(V, H, W, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (V, 3, H, W)).astype(F)


def power_scene(P=48, W=640, H=480, seed=5):
    """large, semi-transparent splats that cover some hundred tiles each: hundreds of work units add into one record.
    Chosen on an MI355X: over five atomic backwards all ten pairs of runs differed, in 961 to 1026 of the 1248 gradient elements
    (two sessions)."""
    rng = np.random.default_rng(seed)
    g = dict(means3D=np.stack([rng.uniform(-0.6, 0.6, P), rng.uniform(-0.4, 0.4, P), rng.uniform(2.0, 4.0, P)], 1).astype(F),
             scales=rng.uniform(0.25, 0.6, (P, 3)).astype(F), rotations=np.tile(np.array([1, 0, 0, 0], F), (P, 1)),
             opacities=rng.uniform(0.05, 0.3, (P, 1)).astype(F), shs=(0.5 * rng.standard_normal((P, 1, 3))).astype(F), sh_degree=0)
    return util.scene_from(g, util.identity_camera(W, H), W, H, bg=(0.1, 0.1, 0.1))


def leaves(g, dev):
    import torch
    L = {k: NC.to_device(g[k], dev).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    L["means2D"] = torch.zeros((g["means3D"].shape[0], 3), device=dev, requires_grad=True)
    return L


# ---- full size --------------------------------------------------------------------------------------------------------------------
FULLSIZE_CONFIGS = {
    # BASELINE.json configs[1]: THuman-256 (200K voxelised), 1080p, inference profile
    "thuman256_1080p": dict(workload="synth-THuman-256", W=1920, H=1080, profile="inference", view=0),
    # configs[2]: THuman-800K, 1080p, training profile (the headline workload)
    "thuman800k_1080p": dict(workload="synth-THuman-800K", W=1920, H=1080, profile="training", view=3),
    # configs[4]: 2M-point sampled mesh, 4K
    "mesh2m_4k": dict(workload="synth-mesh-2M", W=3840, H=2160, profile="training", view=5),
}


def fullsize_scene(cfg, voxel_exact=False):
    from pcrender import camera, synth
    cloud = synth.make_cloud(cfg["workload"], seed=0)
    g = synth.make_gaussians(cloud, profile=cfg["profile"], seed=1)
    if voxel_exact:
        g["means3D"] = cloud["means3D"].copy()
    v = camera.circle_views(12, fov_deg=45.0, width_px=cfg["W"], height_px=cfg["H"])[cfg["view"]]
    return util.scene_from(g, v, cfg["W"], cfg["H"], bg=(1, 1, 1))


# ---- finite differences -----------------------------------------------------------------------------------------------------------
def fd_single_gaussians(s, dev, g, dL, field, grad_key, rel_eps, K, rng, tag, in_plane=False):
    """Central differences of loss = sum(image * dL) of the HIP forward, perturbing ONE Gaussian at a time along a random
    direction in ONE input tensor, against the analytic directional derivative of that Gaussian.  Returns (slope of the
    least-squares line FD = slope * analytic, Pearson correlation) over K Gaussians.  in_plane: position steps keep the
    view-space depth (steps in depth reorder overlapping splats, a jump no gradient describes)."""
    from oracle.oracle import Scene
    base = getattr(s, field)
    gk = g[grad_key].astype(np.float64).reshape(base.shape)
    strength = np.linalg.norm(gk, axis=1)
    cand = np.nonzero(strength > np.quantile(strength[strength > 0], 0.5))[0]   # Gaussians that matter to this loss
    pick = rng.choice(cand, size=min(K, cand.size), replace=False)
    fd, an = [], []
    r2 = np.array([s.viewmatrix[2], s.viewmatrix[6], s.viewmatrix[10]], np.float64)   # view direction (row 2 of the rotation)
    for k in pick:
        d = rng.standard_normal(base.shape[1])
        if field == "means3D" and in_plane:
            d -= r2 * (d @ r2) / (r2 @ r2)
        d /= np.linalg.norm(d)
        step = rel_eps * (np.abs(s.scales[k]).mean() if field != "rotations" else 1.0)
        vals = []
        thetas = []
        for sign in (+1, -1):
            arr = base.copy()
            arr[k] = (base[k].astype(np.float64) + sign * step * d).astype(np.float32)
            kw = dict(means3D=s.means3D, opacities=s.opacities, scales=s.scales, rotations=s.rotations)
            kw[field] = arr
            s2 = Scene(W=s.W, H=s.H, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=s.bg, viewmatrix=s.viewmatrix,
                       projmatrix=s.projmatrix, campos=s.campos, shs=s.shs, sh_degree=s.sh_degree, **kw)
            img = util.run_product(s2, dev, light=True)[0]["out_color"].astype(np.float64)
            vals.append(float((img * dL).sum()))
            thetas.append(arr[k].astype(np.float64))
        fd.append(vals[0] - vals[1])
        an.append(float(gk[k] @ (thetas[0] - thetas[1])))       # the float32 values actually rendered define the step
    fd, an = np.asarray(fd), np.asarray(an)
    slope = float((fd * an).sum() / (an * an).sum())
    corr = float(np.corrcoef(fd, an)[0, 1])
    print("%s %s: %d Gaussians, FD = %.4f x analytic, correlation %.5f" % (tag, field, fd.size, slope, corr))
    return slope, corr
