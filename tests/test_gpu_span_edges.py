"""The row spans of the footprint clipping on the device's own arithmetic (csrc/tile_cull.hpp clip_rect_to_footprint as k_preprocess
runs it -- v_sqrt_f32, the packing of the spans into the Splat line -- and binning.hip k_duplicate's emission from them), on the
scenes of tests/span_cases.py: thin rotated splats whose opacity puts the best pixel of a tile DIAGONAL to the centre tile within a
hair of the alpha = 1/255 cut, means in the border tiles and off the image, clipped boxes of 8 / 9 rows and 15 / 16 columns.  A span
that left such a tile out would lose a blended pixel: the image, final_T and n_contrib would differ from the reference build's,
which evaluates every entry of its full lists at every pixel.  tests/test_cpu_span_cases.py holds the census of the scenes on the
CPU; tests/test_cpu_footprint_clip.py the same arithmetic on the host against a brute-force walk of the pixels."""
import numpy as np
import pytest
import torch

import native_calls as NC
import span_cases as SC
import util
from util import run_product

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", SC.VARIANTS)
def test_spans_of_thin_splats_grazing_the_alpha_cut(variant, oracle, gpu_device):
    from diff_gaussian_rasterization import _native as N
    ref = util.strict_reference()
    c = SC.case(variant, oracle)
    s = c["scene"]
    tag = "span scene %d" % variant
    dL = util.seeded_dL(s)
    r, gr = ref.forward_backward(s, dL)
    # --- how close to the cut the targets are on the reference build's own float32 means / conics (bit for bit the oracle's)
    d = SC.census(r, c)
    print("%s: %s" % (tag, d))
    assert d["just_in"] >= 100 and d["just_out"] >= 100 and d["hair"] >= 40 and d["blended"] >= 0.9, d
    # --- the reference's full lists: everything bit for bit, lists and n_contrib included
    full, _ = run_product(s, gpu_device, dL_dpix=dL)
    assert full["R"] == r["R"]
    for k in ("radii", "tiles_touched", "vals", "keys", "ranges", "n_contrib"):
        np.testing.assert_array_equal(full[k], r[k], err_msg="%s %s" % (tag, k))
    # --- the product's default, clipped lists with row spans: what the API returns bit for bit the reference build's, the lists the
    # reference's with dead pairs removed (replayed pixel by pixel), n_contrib the same Gaussian through the shorter lists
    clip, gc = run_product(s, gpu_device, dL_dpix=dL, reference_lists=False)
    assert clip["R"] == r["R"]
    np.testing.assert_array_equal(clip["radii"], r["radii"])
    assert clip["final_T"].tobytes() == r["final_T"].tobytes(), tag + ": final_T"
    assert clip["out_color"].tobytes() == r["out_color"].tobytes(), tag + ": out_color"
    kept, total = util.check_clipped_equivalent(full, clip, tag, check_dead=True)
    gr = dict(gr)
    gr["dL_dopacity"] = gr["dL_dopacity"].reshape(gc["dL_dopacity"].shape)
    util.check_grads(gc, gr, tag + ", clipped lists")
    # --- were the spans in play?  A Gaussian that emits fewer tiles than the bounding box of its emitted tiles went through them
    count, cols, rows = SC.emitted_boxes(clip["keys"], clip["vals"], s.P)
    spanned = int((count < cols * rows).sum())
    print("%s: clipped lists keep %d of %d pairs; %d of %d visible splats emit less than their tiles' bounding box; boxes of 8 rows: %d, "
          "9 rows: %d, 15 columns: %d, 16 columns: %d" % (tag, kept, total, spanned, clip["visible"], int(((rows == 8) & (cols <= 15)).sum()),
                                                           int((rows == 9).sum()), int(((cols == 15) & (rows <= 8)).sum()), int((cols == 16).sum())))
    assert spanned >= clip["visible"] // 4, "the spans were not in play"
    assert ((count == cols * rows) | ((rows <= 8) & (cols <= 15))).all(), "spans beyond the encoding's 8 rows x 15 columns"
    # --- the same cloud as a batch of two views: each view's lists are those of its single-view call
    with NC.reference_lists(False):
        args = NC.scene_args(c["scenes"], gpu_device)
        run = N.rasterize_gaussians_batch(*args, need_backward=False)
        V = len(c["scenes"])
        for v in range(V):
            R1, c1, r1, g1, b1, i1 = N.rasterize_gaussians(*NC.one_view(args, v), need_backward=False)
            assert R1 == run[0][v] and torch.equal(c1, run[1][v]) and torch.equal(r1, run[2][v]), (tag, v)
            for name in ("LIST_PAIRS", "POINT_LIST", "POINT_LIST_KEYS", "RANGES", "N_CONTRIB", "FINAL_T"):
                a = N.query(name, s.P, s.W, s.H, R1, run[3], run[4], run[5], view=v, n_views=V)
                b = N.query(name, s.P, s.W, s.H, R1, g1, b1, i1)
                assert torch.equal(a, b), (tag, v, name)
            if v == 0:
                assert c1.cpu().numpy().tobytes() == r["out_color"].tobytes()
                assert np.array_equal(N.query("POINT_LIST", s.P, s.W, s.H, R1, g1, b1, i1).cpu().numpy().view(np.uint32), clip["vals"])
            else:
                pairs = int(N.query("LIST_PAIRS", s.P, s.W, s.H, R1, g1, b1, i1)[0])
                assert 0 < pairs < R1, "view %d: nothing clipped" % v
                r2 = ref.forward(c["scenes"][v])
                assert R1 == r2["R"] and c1.cpu().numpy().tobytes() == r2["out_color"].tobytes(), "view %d against the reference build" % v
                assert N.query("FINAL_T", s.P, s.W, s.H, R1, g1, b1, i1).cpu().numpy().tobytes() == r2["final_T"].tobytes()
