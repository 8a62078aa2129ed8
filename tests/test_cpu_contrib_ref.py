"""The host reference of the contribution statistics (tests/contrib_ref.py) on its own, without a GPU: the numpy restatement of the walk
against cases worked out by hand, its sums against the plain-C oracle's float64 sums on every case, and the condition every case has to
meet -- at most 2 % of the visible Gaussians with an open bracket."""
import numpy as np
import pytest

import contrib_ref as R

ALL = R.CASES + R.WEIGHTED


@pytest.mark.parametrize("name", ["one", "two"])
def test_restatement_against_hand_values(name):
    """one Gaussian, then two overlapping, on a 16 x 16 image: sum, maximum, count and dominant count pixel by pixel in float64"""
    c = R.case(name)
    fwd = c["ref"]["fwd"][0]
    assert list(fwd["ranges"].reshape(-1)) == [0, len(c["scenes"][0].means3D)]
    hand = R.hand_values(fwd, 16, 16)
    wk = R.walk(fwd, 16, 16)
    assert wk["L"] == len(hand)
    for i, (s, mx, n, dom) in enumerate(hand):
        assert n > 0 and wk["count_lo"][i] == wk["count_hi"][i] == n
        assert wk["dom_lo"][i] == wk["dom_hi"][i] == dom
        assert wk["max_lo"][i] == wk["max_hi"][i] and abs(wk["max_lo"][i] - mx) <= 6 * 2.0 ** -24 * mx
        assert abs(wk["sum"][i] - s) <= 6 * 2.0 ** -24 * s
    if name == "two":
        # the nearer Gaussian is first in the list and keeps its values of the one-Gaussian case; the farther one sees T = 1 - alpha
        one = R.hand_values(R.case("one")["ref"]["fwd"][0], 16, 16)[0]
        assert hand[0][:3] == one[:3] and hand[0][3] < one[3] and hand[1][3] > 0
        assert sum(h[3] for h in hand) == len({(x, y) for x in range(16) for y in range(16)} & _covered(fwd))


def _covered(fwd):
    """pixels of the 16 x 16 image some Gaussian reaches with alpha >= 1/255 (float64)"""
    out = set()
    for i in range(int(fwd["P"])):
        mx, my = (float(v) for v in fwd["means2D"][i])
        A, B, C, o = (float(v) for v in fwd["conic_opacity"][i])
        for y in range(16):
            for x in range(16):
                dx, dy = mx - x, my - y
                p = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
                if p <= 0 and min(0.99, o * np.exp(p)) >= 1 / 255:
                    out.add((x, y))
    return out


@pytest.mark.parametrize("name", ALL)
def test_restatement_sum_against_the_oracle(name):
    """the nominal walk's float64 sum of its float32 weights against the oracle's float64 sum: the per-term chain, (L + 5) 2^-24, plus
    the possible contributions"""
    ref = R.case(name)["ref"]
    bar = (ref["L"] + 5) * 2.0 ** -24 * ref["sum"] + ref["slack"]
    err = np.abs(ref["walk_sum"] - ref["sum"])
    assert (err <= bar).all(), "%s: worst %.3g x the bar" % (name, (err / np.maximum(bar, 1e-300)).max())
    assert (ref["sum"][ref["count_lo"] > 0] > 0).all() and not ref["sum"][ref["count_hi"] == 0].any()
    if R.case(name)["weights"] is None:
        assert np.array_equal(ref["sum"], ref["sum_plain"])
        assert abs(ref["sum"].sum() - ref["opacity_sum"]) <= (ref["L"] + 5) * 2.0 ** -24 * ref["opacity_sum"]
    else:
        assert (ref["sum"] <= ref["sum_plain"]).all() and ref["sum"].sum() < 0.95 * ref["sum_plain"].sum()


@pytest.mark.parametrize("name", ALL + ("random2000_cov3d",))
def test_at_most_two_percent_of_the_visible_gaussians_have_an_open_bracket(name):
    c = R.case("random2000", use_cov3d=True) if name == "random2000_cov3d" else R.case(name)
    ref = c["ref"]
    assert ref["visible"].any() and (ref["count_hi"] > 0).any()
    assert R.uncertain_fraction(ref) <= R.CAP, "%s: %.2f %% of the visible Gaussians have lo != hi" % (name, 100 * R.uncertain_fraction(ref))
    assert (ref["count_lo"] <= ref["count_hi"]).all() and (ref["dom_lo"] <= ref["dom_hi"]).all() and (ref["max_lo"] <= ref["max_hi"]).all()
    assert (ref["dom_hi"] <= ref["count_hi"]).all() and not ref["count_hi"][~ref["visible"]].any()


def test_the_cases_reach_what_they_are_for():
    r = R.case("stack300")["ref"]
    assert r["L"] == 300 and (r["count_lo"] > 0).all()                        # more than four staging rounds, nobody stops
    r = R.case("opaque70")["ref"]
    assert r["L"] == 70 and (r["count_lo"][:2] == 256).all() and not r["count_hi"][2:].any() and not r["max_hi"][2:].any()
    r = R.case("behind")["ref"]
    assert (~r["visible"]).sum() >= 10 and not r["count_hi"][~r["visible"]].any()
    r = R.case("partial_40x24")["ref"]
    assert r["count_lo"][0] == 40 * 24                                        # the wide Gaussian reaches every pixel of all six tiles
    m = R.case("views3_random")["weights"]
    assert np.isnan(m).sum() == 2 and (m < 0).sum() > 10
    a, b = R.case("views3")["ref"], R.case("views3_mask")["ref"]
    assert (b["count_hi"] <= a["count_lo"]).all() and b["count_hi"].sum() < a["count_lo"].sum()


def test_the_checker_catches_what_it_is_for():
    ref = R.case("views3")["ref"]
    good = dict(weight_sum=ref["sum"].astype(np.float32), weight_max=ref["max_lo"].astype(np.float32),
                pixel_count=ref["count_lo"].astype(np.int32), dominant_count=ref["dom_lo"].astype(np.int32))
    R.check(good, ref, "good")
    R.check_total(good["weight_sum"], ref)
    i = int(np.argmax(ref["count_lo"]))
    for k, delta in (("pixel_count", 1), ("dominant_count", -1), ("weight_max", 1e-5), ("weight_sum", 1e-3)):
        bad = {n: v.copy() for n, v in good.items()}
        bad[k][i] = bad[k][i] + type(bad[k][i])(delta) if k != "weight_sum" else bad[k][i] * np.float32(1 + delta)
        with pytest.raises(AssertionError, match=k):
            R.check(bad, ref, "bad")
