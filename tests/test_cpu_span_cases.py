"""Census of the span scenes (tests/span_cases.py) on the CPU oracle: the scenes test_gpu_span_edges.py renders must bracket the
alpha = 1/255 cut closely, on both sides, at tiles diagonal to the splats' centre tiles and at pixels that are really blended, with
thin footprints, means off the image and clipped boxes at the limits of the span encoding -- or the GPU test would pass whatever
the spans did."""
import numpy as np
import pytest

import span_cases as SC


@pytest.fixture(scope="module", params=SC.VARIANTS)
def counted(request, oracle):
    c = SC.case(request.param, oracle)
    d = SC.census(oracle.forward(c["scene"]), c)
    print("variant %d: %s" % (request.param, d))
    return c, d


def test_the_targets_bracket_the_cut(counted):
    c, d = counted
    assert d["visible"] >= 1400 and d["targets"] >= 0.9 * d["visible"]
    assert d["just_in"] >= 100 and d["just_out"] >= 100 and d["hair"] >= 40, d
    assert d["blended"] >= 0.9, "the grazing pixels are mostly terminated before the splat is reached"


def test_the_targets_are_tiles_a_span_decides_about(counted):
    c, d = counted
    # diagonal to the centre tile, inside the image
    t = c["target"][c["targeted"]]
    assert d["diagonal"] == d["targets"]
    assert ((t[:, 0] >= 0) & (t[:, 0] < SC.GX) & (t[:, 1] >= 0) & (t[:, 1] < SC.GY)).all()
    assert d["ratio_above_4"] >= 0.85 * d["visible"] and d["ratio_above_8"] >= 0.3 * d["visible"]      # thin, after the dilation
    assert d["off_image"] >= 100 and d["border"] >= 200
    # the limits of the encoding: 8 rows and 15 columns still get spans, 9 and 16 do not
    assert min(d["rows_8"], d["rows_9"], d["cols_15"], d["cols_16"]) >= 15, d


def test_the_second_view_sees_the_cloud_elsewhere(counted, oracle):
    c, _ = counted
    a, b = oracle.forward(c["scenes"][0]), oracle.forward(c["scenes"][1])
    vis = (a["radii"] > 0) & (b["radii"] > 0)
    shift = (b["means2D"] - a["means2D"])[vis]
    assert vis.sum() >= 1400 and (np.abs(shift) > 0.5).all() and (np.abs(shift) < 16).all()
