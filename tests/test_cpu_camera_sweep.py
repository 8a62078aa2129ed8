"""The camera-gradient sweep (tests/camera_sweep.py, tests/test_gpu_camera_fuzz.py) checked without a GPU:

  * the census, from sizes and options alone: the cases the sweep takes contain what the sweep is there for, so that a later change
    of the generator cannot silently empty it;
  * the yardstick alone -- the arbiter's expressions in float32 -- stays inside the plain bar of camera_cases.hold when both are
    fed the plain-C oracle's float32 render-level sums as stand-in records: the `4 x yardstick` exit of the GPU file is a margin;
  * no visible Gaussian changes sides of the frustum clamp between float64 and float32;
  * camera_cases.hold rejects the results of three kernels that are wrong in ways the sweep is there to find (a neighbouring
    view's records, a dropped block of rows, scale_modifier ignored), each simulated on the host."""
import functools

import numpy as np
import pytest

import batch_cases as BC
import camera_cases as CC
import camera_sweep as CS
import channel_cases as CH
import util

F = np.float32
TALLY = dict(outside=0, live=0, worst=0.0, worst_at=None, cases=0, pairs=0, flips=[])
# (case, view) pairs with a Gaussian on different sides of the frustum clamp in float64 and float32: camera_sweep.clamp_flips finds
# them from the inputs and the GPU file leaves them out of the arbiter comparison.  None at this commit.
CLAMP_FLIPS = []


@functools.lru_cache(maxsize=None)
def _table():
    """per case id: batch_cases.expected plus the options the camera kernels read"""
    out = {}
    for i in CS.ids():
        c = BC.case(i)
        e = dict(BC.expected(i, c))
        g = c["g"]
        e.update(nblk=CS.blocks(e["P"]), mode=c["mode"], use_cov3d=c["use_cov3d"], modifier=c["scale_modifier"], degree=int(g["sh_degree"]),
                 rows=int(g["shs"].shape[1]), fov=c["fov"], writer=CS.writer(i), recolor=CS.recolors(i, c),
                 unnormalised=bool(np.abs(np.linalg.norm(g["rotations"], axis=1) - 1).max() > 0.05))
        out[i] = e
    return out


def test_census():
    t = _table()
    small = {i: e for i, e in t.items() if i < BC.MEDIUM_BASE}
    assert len(small) == 96 and [i - BC.MEDIUM_BASE for i in t if i >= BC.MEDIUM_BASE] == [0, 3, 6]
    assert CC.CAM_ROWS == 1024 and CC.CAM_SUM_THREADS == 256
    # the workgroup remap beyond the identity: seq / V > 0 needs nblk >= 9 at V >= 2; k_camera_sum's second lap nblk > 256
    for i, V, P in ((49, 16, 12000), (80, 4, 12000)):
        assert (t[i]["V"], t[i]["P"]) == (V, P) and t[i]["nblk"] >= 9
    assert any(e["V"] >= 2 and e["nblk"] > 256 for e in t.values())
    assert any(e["V"] >= 2 and e["nblk"] > 2 * 256 for e in t.values())
    assert any(e["V"] >= 2 and e["nblk"] >= 9 and e["nblk"] % 8 for e in t.values())
    for j, V, P, nblk in ((0, 5, 300000, 293), (3, 3, 530000, 518), (6, 17, 70000, 69)):
        e = t[BC.MEDIUM_BASE + j]
        assert (e["V"], e["P"], e["nblk"]) == (V, P, nblk)
    assert {e["V"] for e in t.values()} >= {2, 3, 4, 5, 7, 8, 12, 13, 16, 17, 31, 64, 256}
    sh = [e for e in small.values() if e["mode"] == "sh"]
    assert {e["degree"] for e in sh} == {0, 1, 2, 3}
    assert {(e["degree"], e["rows"]) for e in sh if e["rows"] > (e["degree"] + 1) ** 2} >= {(0, 13), (0, 16), (1, 13), (1, 16), (2, 13), (2, 16)}
    assert any(e["mode"] == "colors" for e in small.values())
    assert any(e["mode"] == "sh" and e["use_cov3d"] and e["degree"] > 0 for e in small.values())
    assert {e["modifier"] for e in small.values()} == {0.6, 1.0, 2.5}
    assert any(e["modifier"] != 1.0 and not e["use_cov3d"] for e in small.values())
    assert any(e["unnormalised"] and not e["use_cov3d"] for e in small.values())
    assert {e["fov"] for e in small.values()} >= {30.0, 45.0, 50.0, 60.0}
    assert any(e["W"] < 16 and e["H"] < 16 for e in small.values())
    assert any(e["V"] >= 3 and set(e["empty"]) >= {0, e["V"] // 2, e["V"] - 1} and len(e["empty"]) < e["V"] for e in small.values())
    for w in CS.WRITERS:
        assert sum(e["writer"] == w for e in t.values()) >= 25, w
    rec = [i for i, e in small.items() if e["recolor"]]
    assert len(rec) >= 6 and all(small[i]["mode"] == "sh" and len(small[i]["empty"]) < small[i]["V"] for i in rec)
    for i in rec:
        shs, D2 = CS.recolor_shs(i, BC.case(i))
        assert D2 != small[i]["degree"] and 0 <= D2 <= 3 and shs.shape[1] >= (D2 + 1) ** 2
    assert {CS.recolor_shs(i, BC.case(i))[1] > 0 for i in rec} == {False, True}
    # the six channels cases: nx 4 and 8, each value layout
    d = [CH.draws(i) for i in CS.CHANNEL_CASES]
    assert len(d) == 6 and {x["nx"] for x in d} == {4, 8} and {x["layout"] for x in d} == {0, 1, 2}
    assert all(i < CH.N_SMALL for i in CS.CHANNEL_CASES)
    assert max(CS.blocks(BC.expected(CH.batch_index(i))["P"]) for i in CS.CHANNEL_CASES) >= 9


def test_views_held():
    """the cut to three views is a rule of V and P alone, and no case of the sweep needs it at this commit"""
    assert CS.views_held(3, 530000) == [0, 1, 2] and CS.views_held(256, 257) == list(range(256))
    assert CS.views_held(12, 800000) == [0, 6, 11] and CS.views_held(2, 1500000) == [0, 1]


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


def _stand_in(s, dL, nthreads=8):
    """(radii, clamp mask, records [P,16] float32) of one view from the plain-C oracle's float32 backward"""
    fwd, g = _oracle().forward_backward(s, dL, exact=False, nthreads=nthreads)
    rec = np.zeros((s.P, 16), F)
    if s.P:
        rec[:, 0:2], rec[:, 2:5], rec[:, 5:8] = g["dL_dmean2D"][:, :2], g["dL_dconic"][:, [0, 1, 3]], g["dL_dcolor"]
    return fwd["radii"], np.asarray(fwd.get("clamped", np.zeros((s.P, 3))), bool), rec


@pytest.mark.parametrize("i", CS.ids())
def test_yardstick_alone_and_clamp_flips(i):
    c = BC.case(i)
    scenes, dL = BC.scenes(c), BC.dL_dpix(c)
    V = len(scenes)
    views = list(range(V)) if V <= 17 else sorted({0, V // 2, V - 1})
    worst = 0.0
    for v in views:
        s = scenes[v]
        radii, mask, rec = _stand_in(s, dL[v])
        if CS.clamp_flips(s, radii):
            TALLY["flips"].append((i, v))
        TALLY["pairs"] += 1
        exact, yard = CS.arbiter(s, radii, mask, rec)
        for name, live, dead in CC.TENSORS:
            x, y = np.asarray(exact[name], np.float64), np.asarray(yard[name], np.float64)
            assert np.isfinite(x).all() and np.isfinite(y).all(), (i, v, name)
            assert (x[dead] == 0).all() and (y[dead] == 0).all()
            if v in c["empty"]:
                assert not x.any() and not y.any(), (i, v, name)
            if np.abs(x).max() == 0:
                continue
            plain = util.GRAD_ABS * np.abs(x).max()
            e = np.abs(y - x)[live]
            TALLY["live"] += len(live)
            TALLY["outside"] += int((e > plain).sum())
            worst = max(worst, float(e.max() / plain))
    TALLY["cases"] += 1
    if worst > TALLY["worst"]:
        TALLY["worst"], TALLY["worst_at"] = worst, i
    print("camera sweep case %d (V=%d P=%d): yardstick at most %.3g of the plain bar over %d views" % (i, V, scenes[0].P, worst, len(views)))


def test_yardstick_stays_inside_the_plain_bar():
    """closing test (same process): at most 1 in 1000 live entries of the float32 yardstick lies outside the plain bar, and the
    (case, view) pairs with a frustum-clamp flip are the listed ones, at most 1 % of all"""
    if TALLY["cases"] == 0:
        pytest.skip("no case of the sweep ran in this process")
    print("camera sweep, yardstick alone: %(outside)d of %(live)d live entries outside the plain bar over %(cases)d cases, "
          "worst %(worst).3g x the bar (case %(worst_at)s); clamp flips in %(flips)s of %(pairs)d (case, view) pairs" % TALLY)
    assert TALLY["outside"] * 1000 <= TALLY["live"], TALLY
    if TALLY["cases"] == len(CS.ids()):
        assert sorted(TALLY["flips"]) == sorted(CLAMP_FLIPS), TALLY["flips"]
    assert len(CLAMP_FLIPS) * 100 <= max(TALLY["pairs"], 1)


# ---- the checker can fail -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _checker_case():
    """batch case 3 (V = 5, P = 4097: five blocks of rows; modifier 0.6, scales and unnormalised rotations, SH degree 2): views 0 and 1
    with their stand-in records, the arbiter and the yardstick of view 0"""
    c = BC.case(3)
    assert c["scale_modifier"] == 0.6 and not c["use_cov3d"] and c["g"]["means3D"].shape[0] > 3 * CC.CAM_ROWS
    scenes, dL = BC.scenes(c), BC.dL_dpix(c)
    state = [_stand_in(scenes[v], dL[v]) for v in (0, 1)]
    assert (state[0][0][:CC.CAM_ROWS] > 0).sum() > 100
    exact, yard = CS.arbiter(scenes[0], *state[0])
    return scenes, state, exact, yard


def _as_library(s, radii, mask, rec):
    """what a float32 kernel would return from these inputs: the yardstick, as float32 arrays"""
    return {k: np.asarray(a, F) for k, a in CS.arbiter(s, radii, mask, rec)[1].items()}


def test_checker_accepts_the_right_result():
    scenes, state, exact, yard = _checker_case()
    exits, worst = CC.hold(_as_library(scenes[0], *state[0]), exact, yard, "right")
    assert worst <= 1.0


@pytest.mark.parametrize("fault", ["neighbouring_view_records", "dropped_block", "modifier_ignored"])
def test_checker_rejects(fault):
    scenes, state, exact, yard = _checker_case()
    radii, mask, rec = state[0]
    s = scenes[0]
    if fault == "neighbouring_view_records":
        rec = state[1][2]                                 # at_view(grad_rec, gr_stride, vw + 1)
    elif fault == "dropped_block":
        radii = radii.copy()
        radii[:CC.CAM_ROWS] = 0                           # one workgroup's 1024 rows never added
    else:
        s = util.Scene(W=s.W, H=s.H, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=s.bg, means3D=s.means3D, opacities=s.opacities,
                       viewmatrix=s.viewmatrix, projmatrix=s.projmatrix, campos=s.campos, shs=s.shs, sh_degree=s.sh_degree,
                       scales=s.scales, rotations=s.rotations, scale_modifier=1.0)
    with pytest.raises(AssertionError):
        CC.hold(_as_library(s, radii, mask, rec), exact, yard, fault)
