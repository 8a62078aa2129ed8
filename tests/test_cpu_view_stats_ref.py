"""The host reference of gsr_backward_view_stats (tests/view_stats_ref.py) on hand-written records, the checker against the mistakes
the kernel could make -- each simulated on the host and each one caught --, and the scene of the GPU test's semantic point, checked
with the plain-C oracle's per-view backward: on it the sum of the norms and the norm of the sum can be told apart."""
import numpy as np
import pytest

import view_stats_ref as R

F = np.float32


def _hand():
    """3 views x 4 Gaussians: 0 opposite gradients (they cancel in the sum), 1 seen once, 2 never seen, 3 a 3-4-5 triangle per view"""
    rec = np.zeros((3, 4, 16), F)
    rec[0, 0, :2] = (3.0, 4.0)
    rec[1, 0, :2] = (-3.0, -4.0)
    rec[2, 1, :2] = (0.0, -2.0)
    for v in range(3):
        rec[v, 3, :2] = (3.0 * (v + 1), 4.0 * (v + 1))
        rec[v, 3, 5:9] = (0.5 + v, -1.0, 0.25, -7.0 * v)
    rec[:, :, 2:5] = 9.0          # the conic words are nobody's business here
    rec[:, :, 9:] = -1.0
    radii = np.array([[5, 0, 0, 2], [7, 0, 0, 11], [0, 3, 0, 4]], np.int32)
    return rec, radii


def test_reference_on_hand_written_records():
    rec, radii = _hand()
    ref = R.reference(rec, radii)
    assert ref["grad_norm_sum"].tolist() == [10.0, 2.0, 0.0, 30.0] and ref["grad_norm_sum"].dtype == F
    assert ref["visible_views"].tolist() == [2, 1, 0, 3] and ref["visible_views"].dtype == np.int32
    assert ref["max_radius"].tolist() == [7, 3, 0, 11] and ref["max_radius"].dtype == np.int32
    assert ref["mean2D"].shape == (3, 4, 2) and ref["color"].shape == (3, 4, 3) and ref["opacity"].shape == (3, 4)
    assert ref["color"][2, 3].tolist() == [2.5, -1.0, 0.25] and ref["opacity"][:, 3].tolist() == [0.0, -7.0, -14.0]
    # the shares add up to what a backward hands out, where the norms do not: Gaussian 0 cancels
    assert ref["mean2D"].sum(0)[0].tolist() == [0.0, 0.0]
    rows, far = R.norm_gap(rec, radii)
    assert rows.tolist() == [True, False, False, True] and far.tolist() == [True, False, False, False]
    # accumulate: float32(double(old) + sum), counts added, radii maxed; applied twice
    old = (np.array([0.5, 1e-9, 3.0, 2.0 ** 25], F), np.array([4, 0, 9, 1], np.int32), np.array([6, 8, 1, 2], np.int32))
    acc = R.reference(rec, radii, old)
    assert acc["grad_norm_sum"].tolist() == [10.5, 2.0, 3.0, F(2.0 ** 25 + 30.0)] and acc["grad_norm_sum64"][1] == np.float64(F(1e-9)) + 2.0
    assert acc["visible_views"].tolist() == [6, 1, 9, 4] and acc["max_radius"].tolist() == [7, 8, 1, 11]
    twice = R.reference(rec, radii, (acc["grad_norm_sum"], acc["visible_views"], acc["max_radius"]))
    assert twice["grad_norm_sum"].tolist() == [20.5, 4.0, 3.0, F(np.float64(F(2.0 ** 25 + 30.0)) + 30.0)]
    assert twice["visible_views"].tolist() == [8, 2, 9, 7]
    # float64 inside: a term that float32 would lose against the running sum survives until the one rounding
    rec2 = np.zeros((3, 1, 16), F)
    rec2[0, 0, 0], rec2[1, 0, 0], rec2[2, 0, 0] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert R.reference(rec2, np.ones((3, 1), np.int32))["grad_norm_sum"][0] == F(1.0 + 2.0 ** -23)
    # gx^2 overflows float32, not float64
    rec2[:, 0, 0] = 2.0 ** 100
    assert R.reference(rec2, np.ones((3, 1), np.int32))["grad_norm_sum"][0] == F(3 * 2.0 ** 100)


def _random(V=3, P=300, seed=1):
    rng = np.random.default_rng(seed)
    rec = rng.normal(0, 1e-3, (V, P, 16)).astype(F)
    radii = rng.integers(0, 40, (V, P)).astype(np.int32)
    radii[rng.uniform(size=(V, P)) < 0.3] = 0
    rec[radii == 0] = 0.0
    old = (rng.uniform(0, 1e-2, P).astype(F), rng.integers(0, 50, P).astype(np.int32), rng.integers(0, 30, P).astype(np.int32))
    return rec, radii, old


def _outputs(ref):
    return {k: ref[k].copy() for k in R.STATS + R.SHARES}


def test_checker_accepts_the_reference_and_one_ulp():
    rec, radii, old = _random()
    for o in (None, old):
        ref = R.reference(rec, radii, o)
        out = _outputs(ref)
        R.check(out, ref)
        R.check({k: out[k] for k in ("max_radius", "color")}, ref)           # any subset
        # the neighbouring float32 on the side of the float64 value is within the bar, two steps away is not
        x, r = ref["grad_norm_sum64"], ref["grad_norm_sum"]
        side = np.where(x >= r.astype(np.float64), F(np.inf), F(-np.inf)).astype(F)
        near = np.nextafter(r, side)
        R.check(dict(grad_norm_sum=near), ref)
        with pytest.raises(AssertionError, match="1 float32 ulp"):
            R.check(dict(grad_norm_sum=np.nextafter(near, side)), ref)
    with pytest.raises(AssertionError, match="nothing to check"):
        R.check({}, ref)


def test_checker_rejects_each_simulated_mistake():
    rec, radii, old = _random()
    V, P = radii.shape
    ref = R.reference(rec, radii)
    ref_acc = R.reference(rec, radii, old)

    # the norm of the sum instead of the sum of the norms
    out = _outputs(ref)
    g = rec[:, :, :2].astype(np.float64).sum(0)
    out["grad_norm_sum"] = np.sqrt((g ** 2).sum(1)).astype(F)
    with pytest.raises(AssertionError, match="grad_norm_sum"):
        R.check(out, ref)

    # a neighbouring view's records (the statistics are sums over the views and cannot see it: the shares do)
    wrong = R.reference(np.roll(rec, 1, axis=0), np.roll(radii, 1, axis=0))
    R.check({k: wrong[k] for k in R.STATS}, ref)
    for k in R.SHARES:
        with pytest.raises(AssertionError, match=k):
            R.check({k: wrong[k]}, ref)

    # the last, partial block of 256 rows is dropped: its rows keep what the caller's buffers held
    full = (P // 256) * 256
    assert 0 < full < P
    for k in R.STATS + R.SHARES:
        a = ref[k].copy()
        if k in R.STATS:
            a[full:] = 0              # [P]
        else:
            a[:, full:] = np.nan      # [V][P]...
        with pytest.raises(AssertionError, match=k):
            R.check({k: a}, ref)

    # accumulate ignores the old values
    for k in R.STATS:
        with pytest.raises(AssertionError, match=k):
            R.check({k: ref[k]}, ref_acc)

    # max_radius from view 0 alone
    with pytest.raises(AssertionError, match="max_radius"):
        R.check(dict(max_radius=np.maximum(radii[0], 0).astype(np.int32)), ref)
    # ... and the visibility count from it
    with pytest.raises(AssertionError, match="visible_views"):
        R.check(dict(visible_views=(radii[0] > 0).astype(np.int32)), ref)


def test_the_scene_of_the_semantic_point_separates_the_two_norms():
    """V = 3 with opposite cameras (view_stats_ref.scenes), the plain-C oracle's backward view by view: on at least a quarter of the
    Gaussians seen by two or more views, sum_v |g_v| and |sum_v g_v| lie more than 1e-3 apart -- the GPU test asserts the same on
    the library's records"""
    from oracle.oracle import Oracle
    orc = Oracle()
    scs = R.scenes(257, 3)
    rec = np.zeros((3, 257, 16), F)
    radii = np.zeros((3, 257), np.int32)
    for v, (s, dL) in enumerate(zip(scs, R.dLs(scs))):
        fwd, g = orc.forward_backward(s, dL)
        rec[v, :, :2] = g["dL_dmean2D"][:, :2]
        radii[v] = fwd["radii"]
    rows, far = R.norm_gap(rec, radii)
    print("visible in >= 2 views: %d of 257; the two norms differ by > 1e-3 on %d" % (rows.sum(), far.sum()))
    assert rows.sum() >= 100 and 4 * far.sum() >= rows.sum()
    # every camera sees a good part of the cloud, the opposite one also the Gaussians behind the others
    assert (radii > 0).sum(1).min() > 100 and (radii[1, 5::13] > 0).any() and not (radii[0, 5::13] > 0).any()
