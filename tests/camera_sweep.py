"""The randomised sweep of the camera gradients (gsr_backward_cameras) in view batches: what tests/test_gpu_camera_fuzz.py runs on the
GPU and tests/test_cpu_camera_sweep.py checks on the host.  Importable without a GPU.

The two camera kernels are a function of the per-view 64-B gradient records, the forward's radii, the SH clamp mask and the inputs,
and every one of these can be read back.  The sweep therefore feeds tests/fp64_camera.py with the LIBRARY'S OWN records (word 0-1
mean2D, 2-4 conic x / y / w, 5-7 colour) -- in float64 as the arbiter, with dtype = float32 as the yardstick -- and holds the 35
outputs of every view with camera_cases.hold, unchanged.  That isolates csrc/camera_bwd.hip from the render backward's own
rounding (priced by the colour and channels sweeps) and needs no float64 render backward, so it reaches 256 views and 530 000
Gaussians.

  ids / writer / recolors / CHANNEL_CASES   which of batch_cases' (channel_cases') cases the sweep takes and what it does with each
  _prefilled / _cameras                     the call (arguments: native_calls): NaN-filled outputs, a 0xFF-filled scratch block
  records / arbiter / hold_views            records and mask read back, fed to the arbiter, held; exits / live / worst tallied
  views_held / clamp_flips                  the two rules, from the inputs alone, by which a view is not compared"""
import numpy as np

import batch_cases as BC
import camera_cases as CC
import util
from fp64_camera import camera_backward_fp64
from native_calls import follower_args

F = np.float32
N_SMALL = BC.N_SMALL
MEDIUM = (0, 3, 6)                 # indices into batch_cases.MEDIUM: nblk = 293 at V = 5, 518 at V = 3, 69 at V = 17
WRITERS = ("atomic", "deterministic", "train_math")
# indices into channel_cases' small class, (nx, layout): (8, 2) (4, 1) (8, 0, no view scales) (8, 2) (4, 0) (8, 1); batches of 5 to 17
# views, the last one with 12 blocks per view
CHANNEL_CASES = (2, 3, 4, 12, 15, 30)
ARBITER_ROWS = 2000000             # views_held


def ids(n_small=N_SMALL):
    return list(range(min(n_small, N_SMALL))) + [BC.MEDIUM_BASE + j for j in MEDIUM]


def writer(i):
    """the backward that writes the records of case i: it rotates with the case id"""
    return WRITERS[i % 3]


def blocks(P):
    """workgroups of k_camera_partials per view (camera_blocks of csrc/common.hpp)"""
    return (P + CC.CAM_ROWS - 1) // CC.CAM_ROWS


_ELIGIBLE = {}


def _recolor_eligible(i, c=None):
    if i not in _ELIGIBLE:
        c = BC.case(i) if c is None else c
        _ELIGIBLE[i] = c["mode"] == "sh" and len(c["empty"]) < len(c["views"])
    return _ELIGIBLE[i]


def recolors(i, c=None):
    """whether small case i also runs recolor -> backward -> cameras: every eighth of the small cases that evaluate SHs and have a view
    that is not emptied (counted from case 0 on, so the answer does not depend on how many cases run)"""
    if i >= BC.MEDIUM_BASE or not _recolor_eligible(i, c):
        return False
    return sum(_recolor_eligible(k) for k in range(i)) % 8 == 0


def recolor_shs(i, c):
    """(shs [P, rows, 3], active degree) of case i's recolor: seeded, a degree other than the case's, a table of its own width"""
    rng = np.random.default_rng(31000 + i)
    P, D = c["g"]["means3D"].shape[0], int(c["g"]["sh_degree"])
    D2 = (D + 1 + i % 3) % 4
    rows = 16 if (i // 8) % 2 == 0 else (D2 + 1) ** 2
    shs = (0.15 * rng.standard_normal((P, rows, 3))).astype(F)
    shs[:, 0, :] = rng.normal(0.3, 1.2, (P, 3))           # some channels clamp at 0
    return shs, D2


def with_shs(s, shs, degree):
    """the Scene s with another SH table and active degree"""
    return util.Scene(W=s.W, H=s.H, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=s.bg, means3D=s.means3D, opacities=s.opacities,
                      viewmatrix=s.viewmatrix, projmatrix=s.projmatrix, campos=s.campos, shs=shs, sh_degree=degree, scales=s.scales,
                      rotations=s.rotations, cov3D_precomp=s.cov3D_precomp, scale_modifier=s.scale_modifier)


def retry_capacity(pairs):
    """test_gpu_batch_fuzz.py's rule: a capacity between the smallest and the largest per-view pair count (some views overflow the
    arena, others do not), or None where the counts leave no room for one"""
    live = sorted(p for p in pairs if p > 0)
    if len(live) >= 2 and live[-1] - live[0] >= 2:
        cap = live[0] + (live[-1] - live[0]) // 2
        assert live[0] < cap < live[-1]
        return cap
    return None


def views_held(V, P):
    """the views of a batch that are held to the arbiter (the library call always runs all V): all of them up to ARBITER_ROWS rows of
    vectorised numpy per dtype, the first, the middle and the last view beyond"""
    return list(range(V)) if V * P <= ARBITER_ROWS else sorted({0, V // 2, V - 1})


def clamp_flips(s, radii):
    """how many visible Gaussians of the view lie on different sides of the frustum clamp 1.3 tanfov when t_x / t_z and t_y / t_z are
    evaluated in float64 and in float32: there the float32 kernel and the float64 arbiter differentiate different functions (dL/dt_x
    is 0 beyond the clamp), and a (case, view) with such a Gaussian is not compared"""
    idx = np.nonzero(np.asarray(radii) > 0)[0]
    if idx.size == 0:
        return 0
    limx, limy = F(1.3) * F(s.tanfovx), F(1.3) * F(s.tanfovy)
    sides = []
    for dt in (np.float64, np.float32):
        V = s.viewmatrix.astype(dt)
        W3 = np.array([[V[0], V[4], V[8]], [V[1], V[5], V[9]], [V[2], V[6], V[10]]], dtype=dt)
        t = s.means3D[idx].astype(dt) @ W3.T + np.array([V[12], V[13], V[14]], dtype=dt)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            x, y = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
        sides.append(np.stack([x < -dt(limx), x > dt(limx), y < -dt(limy), y > dt(limy)]))
    return int((sides[0] != sides[1]).any(0).sum())


# ---- the call ---------------------------------------------------------------------------------------------------------------
def _prefilled(N, V, P, dev):
    import torch
    out = (torch.full((V, 4, 4), float("nan"), device=dev), torch.full((V, 4, 4), float("nan"), device=dev),
           torch.full((V, 3), float("nan"), device=dev))
    scratch = torch.full((int(N.lib.gsr_camera_grad_bytes(V, P)),), 255, dtype=torch.uint8, device=dev)
    return out, scratch


def _cameras(N, args, radii, geom, V=None):
    """one gsr_backward_cameras call into NaN-filled outputs with a 0xFF-filled scratch block: per view dict of numpy arrays"""
    dev = args[1].device
    V = args[8].shape[0] if V is None else V
    out, scratch = _prefilled(N, V, args[1].shape[0], dev)
    N.backward_cameras(*follower_args(args, radii, geom, V), _out=out, _scratch=scratch)
    dv, dp, dc = (o.cpu().numpy() for o in out)
    assert np.isfinite(dv).all() and np.isfinite(dp).all() and np.isfinite(dc).all(), "an output was left unwritten"
    return [dict(dL_dviewmatrix=dv[v].reshape(16), dL_dprojmatrix=dp[v].reshape(16), dL_dcampos=dc[v]) for v in range(V)]


def _bits(cams):
    return b"".join(np.ascontiguousarray(c[n]).tobytes() for c in cams for n, _, _ in CC.TENSORS)


# ---- records -> arbiter -> hold ---------------------------------------------------------------------------------------------
def records(N, run, P, W, H, V, views, with_mask=True):
    """{view: (records [P,16] float32, clamp mask [P,3] bool)} as the last backward (the last forward or recolor) left them in the
    arenas of `run` = (counts, color, radii, geom, binning, img, ...)"""
    counts, geom, binning, img = run[0], run[3], run[4], run[5]
    out = {}
    for v in views:
        rec = N.grad_records(geom, P, view=v, n_views=V).cpu().numpy()
        mask = np.zeros((P, 3), bool)
        if with_mask:
            mask = N.query("CLAMPED", P, W, H, counts[v], geom, binning, img, view=v, n_views=V).cpu().numpy().astype(bool)
        out[v] = (rec, mask)
    return out


def arbiter(s, radii, mask, rec):
    """(exact, yardstick): tests/fp64_camera.py fed with one view's records, in float64 and in float32"""
    rec = np.asarray(rec)
    conic = np.zeros((rec.shape[0], 4), rec.dtype)
    conic[:, [0, 1, 3]] = rec[:, 2:5]
    with np.errstate(all="ignore"):
        return tuple(camera_backward_fp64(s, radii, mask, rec[:, 0:2], conic, rec[:, 5:8], dtype=dt) for dt in (np.float64, np.float32))


def figures(lib, exact, yard):
    """one line per tensor in which some live entry lies outside the plain bar: the worst |lib - exact| and |yardstick - exact| in
    units of the plain bar, and the worst |lib - exact| / max(plain, 4 |yardstick - exact|) over the entries (camera_cases.hold
    needs <= 1)"""
    out = []
    for name, live, _ in CC.TENSORS:
        x = np.asarray(exact[name], np.float64).reshape(-1)[live]
        if np.abs(x).max() == 0 or not np.isfinite(np.asarray(lib[name], np.float64)).all():
            continue
        plain = util.GRAD_ABS * np.abs(x).max()
        y = np.abs(np.asarray(yard[name], np.float64).reshape(-1)[live] - x)
        e = np.abs(np.asarray(lib[name], np.float64).reshape(-1)[live] - x)
        if (e > plain).any():
            out.append("%s: |lib - exact| %.3g x the plain bar, |yardstick - exact| %.3g x, worst entry at %.3g of its bar"
                       % (name, e.max() / plain, y.max() / plain, (e / np.maximum(plain, 4 * y)).max()))
    return out


def new_tally():
    return dict(exits=0, live=0, worst=0.0, worst_at=None, views=0, skipped=[])


def hold_views(tag, cams, scenes, radii, recs, tally, skip=()):
    """every view of `recs` (records(...)) against the arbiter fed from its records, by camera_cases.hold; the records of the view's
    visible rows are finite.  Views in `skip` (clamp_flips) keep the finiteness and dead-entry checks only.  Returns the exact
    results by view."""
    exact = {}
    for v, (rec, mask) in sorted(recs.items()):
        t = "%s view %d" % (tag, v)
        vis = np.asarray(radii[v]) > 0
        assert np.isfinite(rec[vis][:, :9]).all(), t + ": a record of a visible row is not finite"
        if v in skip:
            for name, _, dead in CC.TENSORS:
                a = np.asarray(cams[v][name], F).reshape(-1)
                assert np.isfinite(a).all() and (a[dead].view(np.uint32) == 0).all(), (t, name)
            tally["skipped"].append(t)
            continue
        x, y = arbiter(scenes[v], radii[v], mask, rec)
        for line in figures(cams[v], x, y):               # (printed before hold asserts: what a miss looked like)
            print("%s %s" % (t, line))
        exits, worst = CC.hold(cams[v], x, y, t)
        tally["exits"] += exits
        tally["live"] += CC.N_LIVE
        tally["views"] += 1
        if worst > tally["worst"]:
            tally["worst"], tally["worst_at"] = worst, t
        exact[v] = x
    return exact
