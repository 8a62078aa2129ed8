"""The channels sweep's case generator (tests/channel_cases.py) without a GPU: its determinism, and the census of the channel
draws against the launch branches of the batches they ride on (tests/batch_cases.expected)."""
import numpy as np

import batch_cases as BC
import channel_cases as CC

# sha256 over every byte of a case: the batch (batch_cases.fingerprint), the channel draws, the values, scales, bg_extra and image
# gradients
PINNED_FINGERPRINTS = {
    4: "2826d31db314f31dcf7cd917639664d780a0d60e5735f38b0fd956b946bb3919",
    20: "f941f77176c8ef929d02f7cca389aecbfdb09f8dae0de7416051f385d6564891",
    47: "0cbc71b99ee98ad0a8b3d66b29873992951b481a8d6c6eb24047b74a316ff693",
}
PAIRS = [(4, 0), (4, 1), (8, 0), (8, 1), (8, 2)]


def test_generator_is_deterministic():
    for i, want in PINNED_FINGERPRINTS.items():
        a, b = CC.case(i), CC.case(i)
        assert CC.fingerprint(a) == CC.fingerprint(b) == want, (i, CC.fingerprint(a))
        assert CC.expected(i, a) == CC.expected(i, b)
    assert CC.fingerprint(CC.case(1)) != CC.fingerprint(CC.case(6)), "the two channel cases on batch case 1 must differ"


def test_cases_have_the_shapes_of_their_layout():
    for i in (1, 2, 3, 9, 24, 47):
        c = CC.case(i)
        V, P, nx, H, W = len(c["batch"]["views"]), c["batch"]["g"]["means3D"].shape[0], c["nx"], c["batch"]["H"], c["batch"]["W"]
        assert nx in (4, 8) and c["layout"] in ((0, 1, 2) if nx == 8 else (0, 1))
        want = {0: [(P, nx)], 1: [(V, P, nx)], 2: [(P, 4), (V, P, 4)]}[c["layout"]]
        assert [a.shape for a in (c["x"] if isinstance(c["x"], tuple) else (c["x"],))] == want, i
        assert c["dense"].shape == (V, P, nx) and c["bg_extra"].shape == (nx,)
        assert c["dpix"].shape == (V, 3, H, W) and c["dx"].shape == (V, nx, H, W)
        assert (c["scale"] is None) == c["no_scale"]
        if c["scale"] is not None:
            allowed = CC.ROUNDED_SCALES if c["scale_class"] == "rounded" else CC.EXACT_SCALES
            assert c["scale"].shape == (V, nx) and np.isin(c["scale"], allowed).all(), i
        # the dense values are what the layout stands for
        if c["layout"] == 0:
            assert all(np.array_equal(c["dense"][v], c["x"]) for v in (0, V - 1))
        elif c["layout"] == 1:
            assert np.array_equal(c["dense"], c["x"])
        else:
            assert np.array_equal(c["dense"][V - 1, :, :4], c["x"][0]) and np.array_equal(c["dense"][:, :, 4:], c["x"][1])


def test_the_list_of_batches():
    assert CC.SMALL_FROM[:6] == [0, 1, 2, 3, 4, 5], "the pinned batch cases lead"
    assert len(CC.SMALL_FROM) == CC.N_SMALL == 48 and all(0 <= j < BC.N_SMALL for j in CC.SMALL_FROM)
    assert sorted(set(CC.SMALL_FROM)) == sorted(CC.SMALL_FROM[:6] + CC.SMALL_FROM[7:]) and CC.SMALL_FROM[6] == 1
    assert [BC.MEDIUM[j] for j in CC.MEDIUM_FROM] == [(5, 300000, 64, 48), (13, 150000, 272, 256), (17, 70000, 112, 96)]
    assert CC.ids(3) == [0, 1, 2] + [CC.MEDIUM_BASE + j for j in range(3)]
    # the medium cases keep the (views per thread, grid rows, views of the last row) of the batches they are cut from
    for j, jb in enumerate(CC.MEDIUM_FROM):
        V, P = BC.MEDIUM[jb][:2]
        assert BC.preprocess_vpt(V, CC.MEDIUM_POINTS.get(j, P)) == BC.preprocess_vpt(V, P), j
    assert BC.preprocess_vpt(5, 262144) == (4, 2, 1) and BC.preprocess_vpt(13, 150000) == (4, 4, 1) and BC.preprocess_vpt(17, 70000) == (2, 9, 1)
    quarter = [CC.draws(i)["scale_class"] == "rounded" for i in CC.ids() if i < CC.MEDIUM_BASE]
    assert sum(quarter) * 4 == len(quarter)


def census(ids):
    out = []
    for i in ids:
        if i < CC.MEDIUM_BASE:
            out.append(CC.expected(i))
        else:                            # (the medium cases: the formulas only, without building their clouds)
            V, P, W, H = BC.MEDIUM[CC.MEDIUM_FROM[i - CC.MEDIUM_BASE]]
            P = CC.MEDIUM_POINTS.get(i - CC.MEDIUM_BASE, P)
            T = ((W + 15) // 16) * ((H + 15) // 16)
            out.append(dict(CC.draws(i), V=V, P=P, W=W, H=H, T=T, dynamic=BC.backward_dynamic(V, T), empty=[], mixed=False))
    return out


def test_census_of_the_default_range():
    exp = census(CC.ids())
    for nx, layout in PAIRS:
        mine = [e for e in exp if (e["nx"], e["layout"]) == (nx, layout)]
        assert any(e["V"] >= 13 for e in mine), "nx=%d layout=%d: no case of 13 or more views" % (nx, layout)
        assert any(e["V"] <= 3 for e in mine), "nx=%d layout=%d: no case of 3 or fewer views" % (nx, layout)
    assert not any(e["nx"] == 4 and e["layout"] == 2 for e in exp)
    for layout in (0, 1, 2):
        mine = [e for e in exp if e["layout"] == layout]
        assert any(e["dynamic"] for e in mine), "layout %d never meets the pulled backward units" % layout
        assert any(not e["dynamic"] for e in mine), "layout %d never meets the static backward grid" % layout
        assert any(e["empty"] for e in mine), "layout %d never meets an empty view" % layout
    assert sum(e["no_scale"] for e in exp) >= 2
    assert any(e["mixed"] and e["nx"] == 8 and e["layout"] == 2 for e in exp), "no slab of mixed pass counts in the split layout"
    assert any(e["W"] * e["H"] < 64 for e in exp)
    assert {1, 63, 65} <= {e["P"] for e in exp}
    print("census: %d cases; (nx, layout) %s; without view scales %d; rounded scales %d; dynamic %s; empty views in %d; mixed %d" % (
        len(exp), {p: sum((e["nx"], e["layout"]) == p for e in exp) for p in PAIRS}, sum(e["no_scale"] for e in exp),
        sum(e["scale_class"] == "rounded" for e in exp), [(e["nx"], e["layout"]) for e in exp if e["dynamic"]],
        sum(bool(e["empty"]) for e in exp), sum(e["mixed"] for e in exp)))
