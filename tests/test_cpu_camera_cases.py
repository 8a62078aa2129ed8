"""The seeded scenes of tests/test_gpu_camera_backward.py (tests/camera_cases.py), checked without a GPU: each contains what it is named
for, and the float32 yardstick of the GPU file's bar -- the arbiter's expressions in single precision, fed with the plain-C oracle's
float32 render-level sums -- lies inside the plain bar on every entry, so the `4 x yardstick` exit there is a margin and no need."""
import numpy as np
import pytest

import camera_cases as CC
import util


@pytest.mark.parametrize("name", CC.ARBITER_CASES + ("channels",))
def test_yardstick_is_inside_the_plain_bar(name):
    ref = CC.reference(name)
    worst = 0.0
    for v, (exact, yard) in enumerate(zip(ref["exact"], ref["yard"])):
        for tname, live, dead in CC.TENSORS:
            x = np.asarray(exact[tname], np.float64)
            y = np.abs(np.asarray(yard[tname], np.float64) - x)
            assert np.isfinite(x).all() and (x[dead] == 0).all() and (np.asarray(yard[tname])[dead] == 0).all()
            if np.abs(x).max() == 0:
                assert (y == 0).all(), (name, v, tname)
                continue
            plain = util.GRAD_ABS * np.abs(x).max()
            worst = max(worst, float(y[live].max() / plain))
            assert (y[live] <= plain).all(), "%s view %d %s: yardstick %.3g off, plain bar %.3g" % (name, v, tname, y[live].max(), plain)
    print("%s: yardstick at most %.3g of the plain bar" % (name, worst))


def test_branch_census():
    """each scene really contains what it is named for"""
    assert CC.EDGE_SIZES == (CC.CAM_ROWS - 1, CC.CAM_ROWS, CC.CAM_ROWS + 1, 2 * CC.CAM_ROWS + 3)
    assert CC.MANY_PARTIALS_P // CC.CAM_ROWS + 1 == CC.CAM_SUM_THREADS + 2     # two threads of k_camera_sum take a second partial
    src = open(util.PKG + "/csrc/common.hpp").read()
    assert "CAM_THREADS = %d;" % CC.CAM_SUM_THREADS in src and "CAM_G = %d;" % (CC.CAM_ROWS // CC.CAM_SUM_THREADS) in src
    one = CC.reference("one")
    assert one["scenes"][0].P == 1 and len(one["scenes"]) == 1 and one["f64"].views()[0]["fwd"]["radii"][0] > 0
    assert np.abs(one["exact"][0]["dL_dcampos"]).max() > 0
    for n in CC.EDGE_SIZES:
        ref = CC.reference("edges_%d" % n)
        assert ref["scenes"][0].P == n and len(ref["scenes"]) == 3
        for w in ref["f64"].views():
            vis = w["fwd"]["radii"] > 0
            assert vis[-1] and vis[:CC.CAM_ROWS].any()                  # the last row, the one at the block's edge, counts
    for name in ("mixed_sh0", "mixed_sh3", "mixed_precomp"):
        ref = CC.reference(name)
        views = ref["f64"].views()
        assert (views[1]["fwd"]["radii"] <= 0).all()                    # the view that looks away sees nothing
        for tname, _, _ in CC.TENSORS:
            assert (np.asarray(ref["exact"][1][tname]) == 0).all()
        for v in (0, 2):
            out, behind, col = CC.census(ref["scenes"][v], views[v]["fwd"])
            assert out.size and behind.size, (name, v)
            assert (col.size > 0) == (name != "mixed_precomp"), (name, v)
        dC = np.abs(ref["exact"][0]["dL_dcampos"]).max()
        assert (dC > 0) == (name == "mixed_sh3"), name                  # degree 0 and precomputed colours: exactly zero
    ch = CC.reference("channels")
    assert len(ch["scenes"]) == 2 and ch["scenes"][0].P > 0
