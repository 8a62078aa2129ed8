"""Randomised sweep of the EXTRA-CHANNEL calls in view batches (gsr_forward_batch_channels, gsr_forward_batch_channels_train,
gsr_backward_batch_channels) under the discipline of tests/test_gpu_batch_fuzz.py: the seeded cases of tests/channel_cases.py (view
batches of tests/batch_cases.py -- 2 to 256 views, 1 x 1 and 7 x 5 images, clouds at the edges of a wave / workgroup / slice, empty
first / middle / last views, slabs of mixed depth-sort pass counts, the views-per-thread ladder of k_preprocess, the pulled work
units of k_render_backward -- with nx in {4, 8}, the three value layouts, view scales present or absent), per case

  * inference forward (need_backward = False): out_color, radii and the counts bit for bit those of the plain colour call;
    out_extra[v], per group of three channels, bit for bit the reference build's own forward of view v with colors_precomp =
    float32(values x scale) and the group's bg_extra as background.  That holds for BOTH scale classes: k_render_forward<NX>
    multiplies a staged value by its view's factor first (render_fwd.hip, `e0 *= xs0` where the entry is staged) and by alpha and T
    afterwards ((e x alpha) x T, the reference's c x alpha x T), so the rounded scales {-1.7, 3.0, 0.3} must reproduce
    float32(value x scale) term for term as well.  Empty views: bg_extra, exactly;
  * training forward (need_backward = True): the four outputs bit for bit those of the inference forward;
  * channels backward: the eight per-Gaussian gradients against the same sums made of the reference build's colour backwards
    (test_gpu_channels_fp64._ref_decomposition), through the counted ladder of tests/grad_ladder.py with the channels float64
    (grad_ladder.ChannelsFloat64 over fp64_channels.channels_backward_fp64_scenes) as the arbiter; dL_dextra_values in the layout's
    own shape against fold_extra of the float64 result; per view, the colour / opacity records and (layouts 1 and 2) the view's own
    block of dL_dextra_values against that view's float64 (a view written with a neighbour's stride is invisible in the sums);
    empty views: records and blocks exactly zero;
  * partial retry: a capacity between the smallest and the largest per-view pair count gives the same bits through the resumed
    forward with its grown extra-state block, and its arenas serve the same backward comparison;
  * colour backward on the arenas of the channels forward: gsr_backward_batch, and on small cases gsr_backward_batch_det twice
    (bit-identical), inside util.check_grads of a colour backward after a plain forward;
  * cases whose index is divisible by 4: the channels backward in the moments modes 0 and 1 as well, through the same ladder.

Checked beforehand without a GPU: hold_to_reference was run on all 48 small cases and the medium cases with the same decomposition
made of the plain-C oracle's float32 backwards in place of the kernel's gradients, float64 as the reference: 51 cases, 4.6 M rows, no
failing row and no exit of the ladder; dL_dextra of that decomposition lay at most 2.4e-6 of max|g| from float64, so dL_dextra was
left as drawn (uniform in [-1, 1], undamped).  One draw was dropped on that evidence: batch case 40 was first in the list, and one
of its splats left through the conditioning exit there (float32 chain 0.56 from float64 in dL_drot where the row bar allows far
less); on the GPU two atomic colour backwards of that batch then differed by 1.75x the element bar of util.check_grads in dL_dscale
in one of two sessions, by the order in which the float atomics arrive.  Batch case 52 (the same image, 12 views) took its place.

GSR_CHANNEL_FUZZ_CASES sets the number of small cases (default 48); the medium cases always run."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import batch_cases as BC
import channel_cases as CC
import util
from fp64_channels import _groups, fold_extra
from fp64_pins import ref_decomposition as _ref_decomposition, rel_err as _err
from grad_ladder import (MAX_CASE_FRACTION, MAX_CASE_FRACTION_REF_TOO, MAX_ROW_FRACTION, MAX_ROW_FRACTION_REF_TOO, ChannelsFloat64,
                         assert_exits_stay_rare, hold_to_reference, new_tally)
from native_calls import channels_backward_args, moments, scene_args as _args, to_device as _t
from sweep_support import records_backward as _backward, same_bits as _same_bits

pytestmark = pytest.mark.gpu

N_SMALL = int(os.environ.get("GSR_CHANNEL_FUZZ_CASES", str(CC.N_SMALL)))
NAMES = util.GRAD_NAMES
F = np.float32
# the exits of the gradient ladder over this file's comparisons (every channels backward -- first arenas, retried arenas, moments
# modes 0 and 1 -- is a comparison of its own), capped by the closing test with the constants of test_gpu_fuzz.py
TALLY = new_tally()
STATS = dict(cases=0, views=0, view_counts=set(), retry_eligible=0, partial_retries=0, dynamic_cases=0, depth_passes_seen=set(),
             pairs={}, no_scale=0, rounded=0, empty_views=0, moments_runs=0, deterministic_runs=0, slowest=(0.0, None),
             worst=dict(extra=0.0, opacity=0.0, colour=0.0, mean2D=0.0, conic=0.0),
             worst_ref=dict(extra=0.0, opacity=0.0, colour=0.0, mean2D=0.0, conic=0.0))


def _channels_backward(N, args, run, extra, dpix_t, dx_t):
    """one channels backward on the arenas of `run`: the eight gradients, dL_dextra_values (numpy; the split layout: a pair) and the
    per-view records [V, P, 16]"""
    g = N.rasterize_gaussians_backward_channels_batch(*channels_backward_args(args, run, dpix_t, extra, dx_t))
    gp = {n: t.detach().cpu().numpy() for n, t in zip(NAMES, g[:8])}
    gx = tuple(a.cpu().numpy() for a in g[8]) if isinstance(g[8], tuple) else g[8].cpu().numpy()
    P, V = args[1].shape[0], dpix_t.shape[0]
    rec = np.stack([N.grad_records(run[3], P, view=v, n_views=V).cpu().numpy() for v in range(V)])
    return gp, gx, rec


def _flat1(g):
    return np.concatenate([np.asarray(a).reshape(-1) for a in g]) if isinstance(g, tuple) else np.asarray(g).reshape(-1)


def _view_block(gx, layout, v):
    """the part of dL_dextra_values that only view v writes (layouts 1 and 2)"""
    return gx[v] if layout == 1 else gx[1][v]


def _check_extra_grads(tag, gx, want, layout, empty):
    dense = np.stack([w["extra"] for w in want["views"]])
    assert np.isfinite(_flat1(gx)).all(), tag
    util.check_grads({"dL_dextra": _flat1(gx).reshape(-1, 1)}, {"dL_dextra": _flat1(fold_extra(dense, layout)).reshape(-1, 1)}, tag,
                     names=("dL_dextra",))
    if layout == 0:
        return
    for v, w in enumerate(want["views"]):
        a, b = _view_block(gx, layout, v), (w["extra"] if layout == 1 else w["extra"][:, 4:])
        if v in empty:
            assert not a.any(), "%s: dL_dextra_values block of the empty view %d" % (tag, v)
        util.check_grads({"dL_dextra": a.reshape(-1, 1)}, {"dL_dextra": b.reshape(-1, 1)}, "%s view %d block" % (tag, v), names=("dL_dextra",))


def _check_records(tag, rec, want, rv, empty):
    for v, w in enumerate(want["views"]):
        r = rec[v]
        assert np.isfinite(r).all(), (tag, v)
        if v in empty:
            assert not r.any(), "%s: records of the empty view %d" % (tag, v)
        util.check_grads({"opacity": r[:, 8:9], "colour": r[:, 5:8]}, {"opacity": w["opacity"][:, None], "colour": w["colour"]},
                         "%s view %d records" % (tag, v), names=("opacity", "colour"))
        if rv is not None:       # measured, not asserted: the distances the closing test prints
            for k, a in (("opacity", r[:, 8]), ("colour", r[:, 5:8]), ("mean2D", r[:, 0:2]), ("conic", r[:, 2:5])):
                if np.abs(w[k]).max() > 0:
                    STATS["worst"][k] = max(STATS["worst"][k], _err(a, w[k]))
                    STATS["worst_ref"][k] = max(STATS["worst_ref"][k], _err(rv[v][k], w[k]))


@pytest.mark.parametrize("i", CC.ids(N_SMALL))
def test_random_channels_batch_matches_reference_build(i, gpu_device):
    from diff_gaussian_rasterization import _native as N
    t_start = time.time()
    dev = gpu_device
    ref = util.reference_build("strict")
    c = CC.case(i)
    b = c["batch"]
    exp = CC.expected(i, c)
    scenes = BC.scenes(b)
    V, P, W, H, nx, layout = exp["V"], exp["P"], exp["W"], exp["H"], c["nx"], c["layout"]
    tag = "channels case %d (batch %d: V=%d P=%d %dx%d; nx=%d layout=%d scales %s)" % (
        i, CC.batch_index(i), V, P, W, H, nx, layout, "none" if c["scale"] is None else c["scale_class"])
    dense, bgx, dpix, dx = c["dense"], c["bg_extra"], c["dpix"], c["dx"]
    sc1 = np.ones((V, nx), F) if c["scale"] is None else c["scale"]
    args = _args(scenes, dev)
    xt = tuple(_t(a, dev) for a in c["x"]) if isinstance(c["x"], tuple) else _t(c["x"], dev)
    extra = (xt, None if c["scale"] is None else _t(c["scale"], dev), _t(bgx, dev))
    dpix_t, dx_t = _t(dpix, dev), _t(dx, dev)
    small = i < CC.MEDIUM_BASE
    STATS["cases"] += 1
    STATS["views"] += V
    STATS["view_counts"].add(V)
    STATS["pairs"][(nx, layout)] = STATS["pairs"].get((nx, layout), 0) + 1
    STATS["no_scale"] += int(c["scale"] is None)
    STATS["rounded"] += int(c["scale_class"] == "rounded" and c["scale"] is not None)
    STATS["dynamic_cases"] += int(exp["dynamic"])
    STATS["empty_views"] += len(exp["empty"])

    # ---- the reference build: per view the colour run and one colors_precomp run per group of three channels
    images = np.zeros((V, nx, H, W), F)
    rv, gr = _ref_decomposition(ref, scenes, dense, sc1, bgx, dpix, dx, images=images)

    # ---- inference forward
    plain = N.rasterize_gaussians_batch(*args, need_backward=False)
    inf = N.rasterize_gaussians_batch(*args, need_backward=False, extra=extra)
    assert inf[0] == plain[0] and torch.equal(inf[1], plain[1]) and torch.equal(inf[2], plain[2]), tag + ": colour outputs"
    out_x = inf[6].cpu().numpy()
    for v in range(V):
        for ks in _groups(nx):
            assert out_x[v, ks].tobytes() == images[v, ks].tobytes(), "%s: out_extra of view %d, channels %s: %d pixels differ, max %g" % (
                tag, v, ks, int((out_x[v, ks] != images[v, ks]).sum()), np.abs(out_x[v, ks] - images[v, ks]).max())
    for v in exp["empty"]:
        assert inf[0][v] == 0 and np.array_equal(out_x[v], np.broadcast_to(bgx[:, None, None], (nx, H, W))), (tag, v)

    # ---- training forward
    run = N.rasterize_gaussians_batch(*args, need_backward=True, extra=extra)
    pairs = (C.c_int64 * V)()
    assert N.lib.gsr_last_list_pairs(pairs, V) == 0
    pairs = [int(x) for x in pairs]
    assert run[0] == inf[0] and all(torch.equal(run[k], inf[k]) for k in (1, 2, 6)), tag + ": training forward"
    for v in range(V):
        words = N.query("DEPTH_SORT", P, W, H, run[0][v], run[3], run[4], run[5], view=v, n_views=V).cpu().numpy().view(np.uint32)
        STATS["depth_passes_seen"].add(int(words[2]))

    # ---- channels backward: the ladder, dL_dextra_values, the per-view records and blocks
    f64 = ChannelsFloat64(scenes, dense, c["scale"], bgx, dpix, dx, nthreads=16)
    want = f64.result()
    gp, gx, rec = _channels_backward(N, args, run, extra, dpix_t, dx_t)
    hold_to_reference(tag, 4242 + i, gp, gr, f64, TALLY, label="channel fuzz")
    _check_extra_grads(tag, gx, want, layout, exp["empty"])
    _check_records(tag, rec, want, rv, exp["empty"])
    ex64 = np.stack([w["extra"] for w in want["views"]])
    if np.abs(ex64).max() > 0:
        STATS["worst"]["extra"] = max(STATS["worst"]["extra"], _err(_flat1(gx), _flat1(fold_extra(ex64, layout))))
        STATS["worst_ref"]["extra"] = max(STATS["worst_ref"]["extra"], _err(_flat1(fold_extra(np.stack([r["extra"] for r in rv]), layout)),
                                                                            _flat1(fold_extra(ex64, layout))))

    # ---- the moments modes 0 and 1
    if i % 4 == 0:
        with moments(None):
            for mode in (0, 1):
                assert N.lib.gsr_set_backward_moments(mode) == mode
                gpm, gxm, recm = _channels_backward(N, args, run, extra, dpix_t, dx_t)
                STATS["moments_runs"] += 1
                hold_to_reference("%s moments mode %d" % (tag, mode), 4242 + i, gpm, gr, f64, TALLY, label="channel fuzz")
                _check_extra_grads("%s moments mode %d" % (tag, mode), gxm, want, layout, exp["empty"])
                _check_records("%s moments mode %d" % (tag, mode), recm, want, None, exp["empty"])

    # ---- partial retry: some views overflow the arena (and the extra-state block carved from its capacity), others do not
    live = sorted(p for p in pairs if p > 0)
    if len(live) >= 2 and live[-1] - live[0] >= 2:
        STATS["retry_eligible"] += 1
        cap = live[0] + (live[-1] - live[0]) // 2
        assert live[0] < cap < live[-1]
        run2 = N.rasterize_gaussians_batch(*args, need_backward=True, extra=extra, capacity=cap)
        STATS["partial_retries"] += int(run2[4].numel() != V * N.lib.gsr_binning_bytes(cap))      # (the binding grew the arena)
        assert run2[0] == run[0] and all(torch.equal(run2[k], run[k]) for k in (1, 2, 6)), tag + ": retried forward"
        gp2, gx2, rec2 = _channels_backward(N, args, run2, extra, dpix_t, dx_t)
        hold_to_reference(tag + " retried", 4242 + i, gp2, gr, f64, TALLY, label="channel fuzz")
        _check_extra_grads(tag + " retried", gx2, want, layout, exp["empty"])
        _check_records(tag + " retried", rec2, want, None, exp["empty"])

    # ---- colour backward on the arenas of the channels forward (include/gsr.h: it writes the colour's saves as the colour forward does)
    run_p = N.rasterize_gaussians_batch(*args, need_backward=True)
    g_plain, rec_plain = _backward(N, args, run_p, dpix_t, False)
    g_col, rec_col = _backward(N, args, run, dpix_t, False)
    util.check_grads(g_col, g_plain, tag + ": colour backward after the channels forward", names=NAMES)
    for v in exp["empty"]:
        assert not rec_col[v].any(), (tag, v)
    if small:
        n_pairs = max(1, max(pairs))
        d1, dr1 = _backward(N, args, run, dpix_t, True, pairs=n_pairs)
        d2, dr2 = _backward(N, args, run, dpix_t, True, pairs=n_pairs)
        STATS["deterministic_runs"] += 2
        assert _same_bits(d1, d2) and np.array_equal(dr1.view(np.uint32), dr2.view(np.uint32)), tag + ": deterministic, second run"
        util.check_grads(d1, g_plain, tag + ": deterministic colour backward after the channels forward", names=NAMES)
    took = time.time() - t_start
    if took > STATS["slowest"][0]:
        STATS["slowest"] = (took, i)
    print("%s: %.1f s" % (tag, took))


def test_channel_fuzz_escape_hatches_stay_rare():
    """Runs after the sweep (same process): the tally of the gradient ladder's exits and the census actually run."""
    if TALLY["cases"] == 0:
        pytest.skip("no channel fuzz case ran in this process")
    print("channel fuzz tally:", TALLY)
    print("channel fuzz: %(cases)d cases, %(views)d views; %(partial_retries)d of %(retry_eligible)d eligible cases retried with a partly "
          "sufficient arena; %(dynamic_cases)d cases with pulled backward units; %(empty_views)d empty views; %(no_scale)d cases without "
          "view scales, %(rounded)d with rounded ones; %(moments_runs)d backwards in moments modes 0 / 1; %(deterministic_runs)d "
          "deterministic colour backwards" % STATS)
    print("channel fuzz: view counts %s; depth-sort pass counts seen %s; (nx, layout) %s; slowest case %d: %.1f s" % (
        sorted(STATS["view_counts"]), sorted(STATS["depth_passes_seen"]), dict(sorted(STATS["pairs"].items())), STATS["slowest"][1],
        STATS["slowest"][0]))
    print("channel fuzz: worst error against float64 in units of max|g| (the reference decomposition's own): %s" % ", ".join(
        "%s %.2e (%.2e)" % (k, STATS["worst"][k], STATS["worst_ref"][k]) for k in ("extra", "opacity", "colour", "mean2D", "conic")))
    assert_exits_stay_rare(TALLY, MAX_CASE_FRACTION, MAX_ROW_FRACTION, MAX_CASE_FRACTION_REF_TOO, MAX_ROW_FRACTION_REF_TOO)
    if N_SMALL >= CC.N_SMALL:
        assert STATS["partial_retries"] >= 1, "no case was retried with an arena that some views fit into"
        assert STATS["dynamic_cases"] >= 3 and STATS["depth_passes_seen"] >= {1, 2, 3, 4}
