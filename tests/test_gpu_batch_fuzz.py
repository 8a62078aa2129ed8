"""Randomised sweep of VIEW BATCHES (gsr_forward_batch + gsr_backward_batch + gsr_backward_batch_det) under the discipline of
tests/test_gpu_fuzz.py: seeded cases (tests/batch_cases.py: 2 to 256 views, images on both sides of the tile sort's second pass,
clouds at the edges of a wave / workgroup / slice, views that see nothing, slabs whose views need different depth-sort pass
counts, and (V, P) pairs that walk the views-per-thread ladder of k_preprocess with ragged last rows), per case

  * forward with the reference's full lists: every integer output, list, range and forward float of every view bit for bit what
    the reference build (oracle/_ref) gives for that view alone, and the per-view depth-sort control words what its depths imply
    (and, for the slabs, what the host predicted);
  * forward in the default (footprint-clipped) mode: the batch equals V single-view calls bit for bit, private lists included;
  * atomic backward: the gradients against the summed per-view reference-build gradients, through the counted ladder of
    tests/grad_ladder.py (float64 summed over the views is the arbiter); the exits are capped with the fuzz's own constants;
  * the per-view colour / opacity records against that view's float64 records wherever float64 was computed, and on every medium
    case (a view written into another view's record block is invisible in the sums);
  * empty views: the background, records exactly zero;
  * partial retry: a capacity between the smallest and the largest per-view pair count (some views overflow, others do not) gives
    the same bits, and its arenas serve the same backward comparison;
  * deterministic backward (small cases): twice on the first arenas, once on the retried ones, all bit-identical and inside
    util.check_grads of the atomic result.

GSR_BATCH_FUZZ_CASES sets the number of small cases (default 96); the medium cases always run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import batch_cases as BC
import util
from grad_ladder import (MAX_CASE_FRACTION, MAX_CASE_FRACTION_REF_TOO, MAX_ROW_FRACTION, MAX_ROW_FRACTION_REF_TOO, Float64,
                         assert_exits_stay_rare, hold_to_reference, new_tally)
from native_calls import reference_lists, scene_args as _args, to_device as _t
from sweep_support import (check_view_against_reference as _check_view_against_reference, records_backward as _backward,
                           same_bits as _same_bits, view_query as _q)

pytestmark = pytest.mark.gpu

N_SMALL = int(os.environ.get("GSR_BATCH_FUZZ_CASES", str(BC.N_SMALL)))
NAMES = util.GRAD_NAMES
# the exits of the gradient ladder over this file's comparisons (a backward on retried arenas is a comparison of its own: it adds
# to the exits and to the totals alike), capped by test_batch_fuzz_escape_hatches_stay_rare with the constants of test_gpu_fuzz.py
TALLY = new_tally()
STATS = dict(views=0, float64_cases=0, retry_eligible=0, partial_retries=0, deterministic_runs=0, depth_passes_of_mixed_cases={},
             depth_passes_seen=set())


@pytest.mark.parametrize("i", BC.ids(N_SMALL))
def test_random_batch_matches_reference_build(i, gpu_device):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    ref = util.reference_build("strict")
    c = BC.case(i)
    exp = BC.expected(i, c)
    scenes = BC.scenes(c)
    V, P, W, H = exp["V"], exp["P"], exp["W"], exp["H"]
    tag = "batch case %d (V=%d P=%d %dx%d)" % (i, V, P, W, H)
    dL = BC.dL_dpix(c)
    dL_t = _t(dL, dev)
    args = _args(scenes, dev)
    STATS["views"] += V

    # ---- the reference build, one view at a time
    rf, gr = [], None
    for v, s in enumerate(scenes):
        r, g = ref.forward_backward(s, dL[v])
        rf.append(r)
        gr = {k: g[k].astype(np.float64) for k in NAMES} if gr is None else {k: gr[k] + g[k] for k in NAMES}

    # ---- forward with the reference's full lists
    with reference_lists(True):
        full = N.rasterize_gaussians_batch(*args, need_backward=True)
        passes = [_check_view_against_reference(N, "%s view %d" % (tag, v), rf[v], full, v, V, P, W, H, c["mode"]) for v in range(V)]
    STATS["depth_passes_seen"].update(passes)
    if exp["depth_passes"] is not None:
        for v, want in enumerate(exp["depth_passes"]):
            assert want is None or passes[v] == want, "%s view %d: %d depth-sort passes, predicted %d" % (tag, v, passes[v], want)
        if exp["mixed"]:
            STATS["depth_passes_of_mixed_cases"][i] = passes

    # ---- forward in the default mode: the batch equals V single-view calls
    with reference_lists(False):
        run = N.rasterize_gaussians_batch(*args, need_backward=True)
        pairs = (C.c_int64 * V)()
        assert N.lib.gsr_last_list_pairs(pairs, V) == 0
        pairs = [int(x) for x in pairs]
        counts, color, radii, geom, binning, img = run
        assert counts == full[0] and torch.equal(color, full[1]) and torch.equal(radii, full[2]), tag + ": clipped vs full lists"
        for v in range(V):
            one = list(args)
            one[8], one[9], one[16] = args[8][v], args[9][v], args[16][v]
            R1, c1, r1, g1, b1, i1 = N.rasterize_gaussians(*one, need_backward=False)
            assert R1 == counts[v], (tag, v)
            assert torch.equal(c1, color[v]) and torch.equal(r1, radii[v]), (tag, v)
            for name in ("POINT_LIST", "POINT_LIST_KEYS", "RANGES", "N_CONTRIB", "FINAL_T", "TILES_TOUCHED", "LIST_PAIRS"):
                a = _q(N, name, P, W, H, R1, run, v, V)
                b = N.query(name, P, W, H, R1, g1, b1, i1)
                assert torch.equal(a, b), (tag, v, name)
            assert int(_q(N, "LIST_PAIRS", P, W, H, R1, run, v, V)[0]) == pairs[v], (tag, v)

        # ---- empty views: the background
        bg = _t(np.asarray(c["bg"], np.float32), dev).view(3, 1, 1).expand(3, H, W)
        for v in exp["empty"]:
            assert counts[v] == 0 and not radii[v].any() and torch.equal(color[v], bg), (tag, v)

        # ---- atomic backward against the summed reference-build gradients
        f64 = Float64(scenes, dL, nthreads=16)
        gp, rec = _backward(N, args, run, dL_t, False)
        for v in exp["empty"]:
            assert not rec[v].any(), "%s: records of the empty view %d" % (tag, v)
        hold_to_reference(tag, 4242 + i, gp, gr, f64, TALLY, label="batch fuzz")
        if c["kind"] == "medium":
            f64.views()
        if f64._views is not None:
            STATS["float64_cases"] += 1
            for v, w in enumerate(f64.views()):
                assert np.isfinite(rec[v]).all(), (tag, v)
                util.check_grads({"opacity": rec[v][:, 8:9], "colour": rec[v][:, 5:8]},
                                 {"opacity": w["exact"]["dL_dopacity"], "colour": w["exact"]["dL_dcolor"]},
                                 "%s view %d records" % (tag, v), names=("opacity", "colour"))

        # ---- partial retry: some views overflow the arena, others do not
        live = sorted(p for p in pairs if p > 0)
        run2 = None
        if len(live) >= 2 and live[-1] - live[0] >= 2:
            STATS["retry_eligible"] += 1
            cap = live[0] + (live[-1] - live[0]) // 2
            assert live[0] < cap < live[-1]
            run2 = N.rasterize_gaussians_batch(*args, need_backward=True, capacity=cap)
            STATS["partial_retries"] += int(run2[4].numel() != V * N.lib.gsr_binning_bytes(cap))   # (the binding grew the arena)
            assert run2[0] == counts and torch.equal(run2[1], color) and torch.equal(run2[2], radii), tag + ": retried forward"
            gp2, rec2 = _backward(N, args, run2, dL_t, False)
            for v in exp["empty"]:
                assert not rec2[v].any(), "%s: records of the empty view %d (retried arenas)" % (tag, v)
            hold_to_reference(tag + " retried", 4242 + i, gp2, gr, f64, TALLY, label="batch fuzz")

        # ---- deterministic backward
        if c["kind"] == "small":
            n_pairs = max(1, max(pairs))
            d1, dr1 = _backward(N, args, run, dL_t, True, pairs=n_pairs)
            d2, dr2 = _backward(N, args, run, dL_t, True, pairs=n_pairs)
            STATS["deterministic_runs"] += 2
            assert _same_bits(d1, d2) and np.array_equal(dr1.view(np.uint32), dr2.view(np.uint32)), tag + ": deterministic, second run"
            if run2 is not None:
                d3, dr3 = _backward(N, args, run2, dL_t, True, pairs=n_pairs)
                STATS["deterministic_runs"] += 1
                assert _same_bits(d1, d3) and np.array_equal(dr1.view(np.uint32), dr3.view(np.uint32)), tag + ": deterministic, retried arenas"
            util.check_grads(d1, gp, tag + ": deterministic vs atomic", names=NAMES)


def test_batch_fuzz_escape_hatches_stay_rare():
    """Runs after the sweep (same process): how many comparisons / rows needed a fallback of the gradient ladder."""
    if TALLY["cases"] == 0:
        pytest.skip("no batch fuzz case ran in this process")
    print("batch fuzz tally:", TALLY)
    print("batch fuzz: %(views)d views; float64 records checked in %(float64_cases)d cases; %(partial_retries)d of %(retry_eligible)d "
          "eligible cases retried with a partly sufficient arena; %(deterministic_runs)d deterministic backwards" % STATS)
    print("batch fuzz: depth-sort pass counts seen %s; per view in the mixed cases: %s" % (
        sorted(STATS["depth_passes_seen"]), STATS["depth_passes_of_mixed_cases"]))
    assert_exits_stay_rare(TALLY, MAX_CASE_FRACTION, MAX_ROW_FRACTION, MAX_CASE_FRACTION_REF_TOO, MAX_ROW_FRACTION_REF_TOO)
    if N_SMALL >= BC.N_SMALL:
        assert STATS["partial_retries"] >= 1, "no case was retried with an arena that some views fit into"
        assert len(STATS["depth_passes_of_mixed_cases"]) >= 3 and STATS["depth_passes_seen"] >= {1, 2, 3, 4}
