"""The arena contract (include/gsr.h at the arena size functions): arenas need not be initialised, what they
hold between calls is the library's, and NO RESULT OF A CALL DEPENDS ON IT.  The library has no memset launches by design -- a frame's
bookkeeping is cleared inside k_preprocess, and much of the saved state is written only where its reader will look -- and the Python
layer allocates every arena with torch.empty, so in a training loop every frame renders into the bytes of an earlier one.

Every case takes ONE set of arenas (geometry with the gradient records, image, binning at a capacity that holds both frames' lists,
extra state for eight channels at that capacity, the deterministic backward's scratch block), and runs the subject frame's calls
twice:

  clean   the arenas zero-filled immediately before;
  stale   the arenas as the donor frame's calls left them, nothing cleared in between.

Everything the header promises to be repeatable is compared by its bits (arena_cases.differing): images, radii, num_rendered,
gsr_last_list_pairs, the ranges, lists, final_T, n_contrib and clamp mask of every view, out_extra, every gradient of the
deterministic backwards, the gradient records, the cameras' 35 outputs, the view statistics and per-view shares, the order-free
contribution statistics.  The atomic backwards (and weight_sum, a float-atomic sum) are held to the CLEAN run's deterministic
gradients at util.check_grads' bars; no tolerance is introduced here.

WHAT COUNTS AS STALE.  An earlier VALID frame of the same P, W, H on the same arenas (arena_cases.py: a donor that shares what carves
the arenas and differs in cloud, cameras, colours and SH degree), or zeros.  Never an arbitrary byte pattern in the geometry, image,
binning or extra-state arenas, and never a frame of another P: where a stale word is read as an index it is still an index of this
arena, so a dependence shows as wrong bits, not as an access out of bounds.  The scratch block of the deterministic colour backward
keeps the fill its own tests use: 0xFF before the clean run and again before the donor's calls, none of which writes it.

Anchor.  The clean run's forward is held once per frame (pair, subject, V) to the reference build
(sweep_support.check_view_against_reference), so that "clean equals stale" is not the agreement of two wrong results.  Once per
MODULE RUN: frame_after_backward, view_count_change, stage_pair, nothing_visible and depth_sort_ping_pong anchor every frame the
module uses; the other cases render the same frames and do not repeat the comparison, so one of them selected alone (-k) runs
without its anchor.  All calls run with the reference's full lists, so that what
tests/test_cpu_arena_cases.py asserts from the oracle (which tiles empty out, whose lists are longer, which quadrants pass a slice
boundary) holds for the frames rendered here.

Positive control, with no broken kernel involved.  Right before the stale run the arenas are copied; for each region the case is
about, the copy must differ from zero AND from what the clean run left there, read at the subject's layout through gsr_query /
grad_records (ranges, lists, final_T, n_contrib, clamp mask, records) or the byte tensors (the slice-boundary states): the donor
really left something else where the subject's calls read and write.  The counts are printed, with the number of arena bytes in
which the two final states still differ -- bytes the subject never wrote; that number is informative and not asserted.

MEASURED on an MI355X, one module run (17 tests in 3.2 s; the first call carries the library's start-up).  Left: the positive
control, words the donor left that differ from zero and from the clean run's, per region.  Middle: arena bytes in which the final
states of the two runs differ (never written by the subject; not asserted).  Right: duration of the call.
  test                                                 ranges  lists  fin_T n_cont  clamp record   ckpt xstate  |    geom binning   image x_state | call
  frame_after_backward                                    185  17348  27316  22574   4080  78300      0      0  |    5532   52517      56       0 | 0.61 s
  records_after_inference_frame                           185  17348  27316  22574   4080  78300      0      0  |    5759   52517      56       0 | 0.01 s
  inference_after_training_frame                          185  17348  27316  22574   4243  78300      0      0  |  320969   52517      91       0 | 0.01 s
  view_count_change[3-1]                                    9   2952    400    353    512  37686   8018      0  |  518970   42089   12009       0 | 0.01 s
  view_count_change[3-2]                                   18   5912    801    712   1024  70535   7055      0  |  253045   41345    8169       0 | 0.02 s
  view_count_change[1-3]                                    9   2956    400    353    512      0   2122      0  |     198   10203    1437       0 | 0.02 s
  recolor_rewrites_saves                                  185  17348  27316  22574   4243  78300      0      0  |    5899   52517      56       0 | 0.02 s
  channels_state[channels8_then_channels4-main]           185  17348  27316  22574   4080  78300      0      0  |    5769   52517      56       0 | 0.03 s
  channels_state[channels8_then_channels4-deep]            27   8864   1202   1067   1534  78300   2969   8704  |     137     286    4338   32308 | 0.02 s
  channels_state[colour_then_channels8-main]              185  17348  27316  22574   4080  78300      0      0  |    5708   52517      56       0 | 0.02 s
  channels_state[colour_then_channels8-deep]               27   8864   1202   1067   1534  78300   2969      0  |      91     286    4338       0 | 0.02 s
  resume_on_used_binning                                  249  13516  32172  31957   3509  65475      0      0  |     271   16987      33       0 | 0.01 s
  stage_pair                                               59   5781   9856   7526   1333  26100      0      0  |      69    9619      12       0 | 0.01 s
  nothing_visible[main]                                   185  17348  27316  22574   4080  78300      0      0  |    5727   52517      56       0 | 0.01 s
  nothing_visible[culled]                                 185  17353  22576  22576   4243  78300      0      0  |   16596  100052      91       0 | 0.02 s
  depth_sort_ping_pong                                    249  13516  32172  31957   3509  65475      0      0  |     218   16987      33       0 | 0.02 s

WHAT THE CASES FOUND.  No dependence on the arenas' earlier content: on an MI355X every clean / stale comparison held at the first
run.  test_nothing_visible[culled] found something else, in the clean run already: dL_drot of a Gaussian that no view saw was -0 in
its components (k_preprocess_backward pushed the zero covariance sums through the quaternion: x * 0 with x < 0), where include/gsr.h
says zeros and the reference's zero-filled output holds +0.  The kernel now leaves the scale / rotation chain out for such a
Gaussian (csrc/preprocess_bwd.hip, `seen`); the case stays as the regression test.  A deliberately broken library is never run on
the device to show that the cases could fail; the census, the positive control and the host tests of `differing` are that evidence."""
import ctypes as C

import numpy as np
import pytest
import torch

import arena_cases as AC
import native_calls as NC
import sweep_support as SS
import util
from fp64_pins import recolor as _recolor

pytestmark = pytest.mark.gpu

F = np.float32
CAPACITY = {"main": 7000, "culled": 7000, "pingpong": 6000, "deep": 3500}   # pairs per view: both frames' lists and a margin
ANCHORED = set()
REGIONS = ("ranges", "lists", "final_T", "n_contrib", "clamped", "records", "ckpt", "xstate")


@pytest.fixture(autouse=True)
def _full_lists_and_exact_training():
    with NC.reference_lists(True), NC.train_math(0), NC.render_math(0):
        yield


class Frame:
    """the donor ("D") or subject ("S") of a pair on the device: its first V views"""
    def __init__(self, pr, who, dev, V=None):
        self.pr, self.who = pr, who
        self.scenes = AC.scenes(pr, who, V)
        self.V, self.P, self.W, self.H = len(self.scenes), AC.P, pr["W"], pr["H"]
        self.args = NC.scene_args(self.scenes, dev)
        self.dpix = NC.to_device(AC.dL_dpix(pr, who, self.V), dev)
        self.tag = "%s %s V=%d" % (pr["name"], who, self.V)


class Arenas:
    def __init__(self, N, pr, V, dev, capacity=None):
        cap = CAPACITY[pr["name"]] if capacity is None else capacity
        self.geom, self.binning, self.img, self.xstate = NC.alloc_arenas(N, AC.P, pr["W"], pr["H"], V, cap, dev, nx=8)
        n = max(N.lib.gsr_backward_det_bytes(v, AC.P, pr["W"], pr["H"], cap) for v in range(1, V + 1))
        self.scratch = torch.empty((int(n),), dtype=torch.uint8, device=dev)

    def all(self):
        return (self.geom, self.binning, self.img, self.xstate)

    def zero(self):
        for a in self.all():
            a.zero_()
        self.scratch.fill_(0xFF)

    def copy(self):
        return tuple(a.clone() for a in self.all())


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _forward(N, f, A, nb, binning=None, **kw):
    rc, run = NC.forward_on(N, f.args, A.geom, A.binning if binning is None else binning, A.img, nb, **kw)
    assert rc == 0, (f.tag, N.lib.gsr_last_error())
    return run


def _anchor(N, f, run):
    """once per frame: every view of this forward against the reference build's forward of that view"""
    if f.tag in ANCHORED:
        return
    ref = util.reference_build("strict")
    for v, s in enumerate(f.scenes):
        SS.check_view_against_reference(N, "%s view %d" % (f.tag, v), ref.forward(s), run, v, f.V, f.P, f.W, f.H, "sh")
    ANCHORED.add(f.tag)


def _facts(N, f, run, nb, tag=""):
    """what a forward returns and what gsr_query shows of it"""
    V = f.V
    pairs = (C.c_int64 * V)()
    assert N.lib.gsr_last_list_pairs(pairs, V) == 0
    q = lambda name: [SS.view_query(N, name, f.P, f.W, f.H, run[0][v], run, v, V).cpu().numpy() for v in range(V)]  # noqa: E731
    d = {"images": run[1].cpu().numpy(), "radii": run[2].cpu().numpy(), "num_rendered": np.array(run[0], np.int64),
         "list_pairs": np.array(list(pairs), np.int64), "ranges": q("RANGES"), "point_list": q("POINT_LIST"), "final_T": q("FINAL_T"),
         "n_contrib": q("N_CONTRIB")}
    if nb:
        d["clamped"] = q("CLAMPED")
    if len(run) > 6:
        d["out_extra"] = run[6].cpu().numpy()
    return {tag + k: x for k, x in d.items()}


def _records(N, f, run):
    return [N.grad_records(run[3], f.P, view=v, n_views=f.V).cpu().numpy() for v in range(f.V)]


def _det(N, f, run, A, tag="", args=None):
    """the deterministic colour backward into the case's scratch block: (named outputs, the gradient dict)"""
    g = NC.colour_det_backward_on(N, f.args if args is None else args, run, f.dpix, A.scratch)
    d = {tag + k: x for k, x in g.items()}
    d[tag + "records"] = _records(N, f, run)
    return d, g


def _followers(N, f, run, tag="", args=None):
    """cameras, view statistics (accumulate 0, then 1 onto those) and per-view shares of the last backward"""
    dev = run[3].device
    fa = NC.follower_args(f.args if args is None else args, run[2], run[3])
    d = {tag + "cameras": _np(N.backward_cameras(*fa))}
    st = (torch.full((f.P,), 7.0, device=dev), torch.full((f.P,), 3, dtype=torch.int32, device=dev),
          torch.full((f.P,), 5, dtype=torch.int32, device=dev))
    shares = N.backward_view_stats(*fa, accumulate=False, grad_norm_sum=st[0], visible_views=st[1], max_radius=st[2], view_grads=True)
    d[tag + "stats"], d[tag + "shares"] = _np(st), _np(shares)
    N.backward_view_stats(*fa, accumulate=True, grad_norm_sum=st[0], visible_views=st[1], max_radius=st[2])
    d[tag + "stats_accumulated"] = _np(st)
    return d


def _contrib(N, f, run, tag=""):
    """(the order-free contribution statistics, weight_sum: a float-atomic sum, held loosely)"""
    dev = run[3].device
    ws, wm = torch.full((f.P,), 9.0, device=dev), torch.full((f.P,), 9.0, device=dev)
    pc, dc = torch.full((f.P,), 9, dtype=torch.int32, device=dev), torch.full((f.P,), 9, dtype=torch.int32, device=dev)
    N.contrib_stats(*NC.contrib_stats_args(f.args, run), accumulate=False, weight_sum=ws, weight_max=wm, pixel_count=pc, dominant_count=dc)
    return {tag + "contrib": _np((wm, pc, dc))}, {tag + "weight_sum": ws.cpu().numpy().reshape(-1, 1)}


def _atomic(N, f, run):
    return SS.records_backward(N, f.args, run, f.dpix, False)[0]


def _donor_training_frame(N, d, A):
    """the tail every donor ends with unless its case says otherwise: a need_backward forward and an atomic backward"""
    run = _forward(N, d, A, True)
    _atomic(N, d, run)
    return run


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def _regions(N, f, state):
    """the regions of the arenas in `state` (geom, binning, img, xstate) at frame f's layout, as uint32 / uint8 arrays"""
    geom, binning, img, xstate = state
    run = (None, None, None, geom, binning, img)
    q = lambda name: [SS.view_query(N, name, f.P, f.W, f.H, 0, run, v, f.V).cpu().numpy() for v in range(f.V)]  # noqa: E731
    cat = lambda xs, dt: np.concatenate([np.ascontiguousarray(x).reshape(-1).view(dt) for x in xs])             # noqa: E731
    return dict(ranges=cat(q("RANGES"), np.uint32), lists=[x.view(np.uint32) for x in q("POINT_LIST")], final_T=cat(q("FINAL_T"), np.uint32),
                n_contrib=cat(q("N_CONTRIB"), np.uint32), clamped=cat(q("CLAMPED"), np.uint8),
                records=cat([N.grad_records(geom, f.P, view=v, n_views=f.V).cpu().numpy() for v in range(f.V)], np.uint32),
                ckpt=cat([NC.ckpt_region(N, binning, f.V, v).cpu().numpy() for v in range(f.V)], np.uint32),
                xstate=xstate.cpu().numpy()[:xstate.numel() // 4 * 4].view(np.uint32))


def _stale_words(before, clean):
    """per region: the words the donor left that are neither zero nor what the clean run leaves there (lists: the entries that
    differ from the clean run's, and the tail behind them)"""
    out = {}
    for k in REGIONS:
        if k == "lists":
            out[k] = sum(int((a[:min(a.size, b.size)] != b[:min(a.size, b.size)]).sum()) + max(0, a.size - b.size)
                         for a, b in zip(before[k], clean[k]))
        else:
            out[k] = int(((before[k] != 0) & (before[k] != clean[k])).sum())
    return out


def _hold(N, case, f, A, donor, subject, about):
    """subject() on zero-filled arenas and on the arenas donor() leaves: equal bits, loose outputs inside check_grads of the clean
    run's reference gradients; the positive control over the regions `about`"""
    A.zero()
    clean, loose_c, want = subject()
    clean_state = A.copy()
    A.zero()
    donor()
    before = A.copy()
    stale, loose_s, _ = subject()
    stale_state = A.copy()
    words = _stale_words(_regions(N, f, before), _regions(N, f, clean_state))
    left = {n: int((a != b).sum()) for n, a, b in zip(("geom", "binning", "image", "extra_state"), clean_state, stale_state)}
    print("arena case %s [%s]: stale words that differ from zero and from the clean run's: %s; arena bytes that differ after the "
          "two runs: %s" % (case, f.tag, ", ".join("%s %d" % (k, words[k]) for k in REGIONS),
                            ", ".join("%s %d" % kv for kv in left.items())))
    bad = AC.differing(AC.outputs(**clean), AC.outputs(**stale))
    assert not bad, "%s: these outputs depend on what the arenas held before the call: %s" % (case, bad)
    for k in about:
        assert words[k] > 0, "%s: the donor left nothing else in %s: the case does not test what it is about" % (case, k)
    for loose in (loose_c, loose_s):
        for k, got in loose.items():
            util.check_grads(got, want[k], "%s %s" % (case, k), names=tuple(got))
    return clean


def _native():
    from diff_gaussian_rasterization import _native as N
    return N


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def test_frame_after_backward(gpu_device):
    """a training frame, its deterministic backward and all followers after a donor's forward and atomic backward: dirty records,
    emptied tiles, a longer stale list, other visibility, another clamp mask"""
    N, pr = _native(), AC.pair("main")
    d, s, A = Frame(pr, "D", gpu_device), Frame(pr, "S", gpu_device), Arenas(N, pr, 3, gpu_device)

    def subject():
        run = _forward(N, s, A, True)
        _anchor(N, s, run)
        out = _facts(N, s, run, True)
        det, g = _det(N, s, run, A)
        out.update(det)
        out.update(_followers(N, s, run))
        strict, ws = _contrib(N, s, run)
        out.update(strict)
        return out, {"contrib": ws}, {"contrib": ws}

    _hold(N, "frame_after_backward", s, A, lambda: _donor_training_frame(N, d, A), subject,
          ("ranges", "lists", "final_T", "n_contrib", "clamped", "records"))


def test_records_after_inference_frame(gpu_device):
    """the donor's last call is an inference forward in the fast arithmetic: it clears no records and leaves its arithmetic in the
    arena's host record.  The subject's exact training frame, deterministic and atomic backwards"""
    N, pr = _native(), AC.pair("main")
    d, s, A = Frame(pr, "D", gpu_device), Frame(pr, "S", gpu_device), Arenas(N, pr, 3, gpu_device)

    def donor():
        _donor_training_frame(N, d, A)
        with NC.render_math(1):
            _forward(N, d, A, False)

    def subject():
        run = _forward(N, s, A, True)
        out = _facts(N, s, run, True)
        det, g = _det(N, s, run, A)
        out.update(det)
        return out, {"atomic": _atomic(N, s, run)}, {"atomic": g}

    _hold(N, "records_after_inference_frame", s, A, donor, subject, ("records", "clamped", "lists"))


def test_inference_after_training_frame(gpu_device):
    N, pr = _native(), AC.pair("main")
    d, s, A = Frame(pr, "D", gpu_device), Frame(pr, "S", gpu_device), Arenas(N, pr, 3, gpu_device)

    def subject():
        run = _forward(N, s, A, False)
        out = _facts(N, s, run, False)
        strict, ws = _contrib(N, s, run)
        out.update(strict)
        return out, {"contrib": ws}, {"contrib": ws}

    _hold(N, "inference_after_training_frame", s, A, lambda: _donor_training_frame(N, d, A), subject,
          ("ranges", "lists", "final_T", "n_contrib"))


@pytest.mark.parametrize("vd,vs", [(3, 1), (3, 2), (1, 3)])
def test_view_count_change(gpu_device, vd, vs):
    """the deep pair: lists longer than a slice in different tiles, at 512 entries (V = 1) and 1024 (V >= 2); the per-view strides,
    the place of the records and the slice length all follow V"""
    N, pr = _native(), AC.pair("deep")
    d, s, A = Frame(pr, "D", gpu_device, vd), Frame(pr, "S", gpu_device, vs), Arenas(N, pr, 3, gpu_device)

    def subject():
        run = _forward(N, s, A, True)
        _anchor(N, s, run)
        out = _facts(N, s, run, True)
        det, g = _det(N, s, run, A)
        out.update(det)
        out.update(_followers(N, s, run))
        return out, {"atomic": _atomic(N, s, run)}, {"atomic": g}

    # (a single view's records lie where three views have their second geometry arena: nothing of the donor's where the subject's are)
    _hold(N, "view_count_change", s, A, lambda: _donor_training_frame(N, d, A), subject,
          ("ckpt", "lists", "n_contrib") + (("records",) if vd == 3 else ()))


def test_recolor_rewrites_saves(gpu_device):
    """within the subject: forward, backward, need_backward recolor with the SHs at another active degree, deterministic backward;
    then a colours-per-view recolor, deterministic backward and followers -- on clean arenas and on a donor's; the recolored images
    also against fresh forwards with those colours"""
    N, pr, dev = _native(), AC.pair("main"), gpu_device
    d, s, A = Frame(pr, "D", dev), Frame(pr, "S", dev), Arenas(N, pr, 3, dev)
    other = list(s.args)
    other[NC.SH_DEGREE] = 2
    assert s.args[NC.SH_DEGREE] == 1
    cols = NC.to_device(np.random.default_rng(77).uniform(-0.2, 1.2, (s.V, s.P, 3)).astype(F), dev)
    coloured = list(s.args)
    coloured[NC.COLORS], coloured[NC.SHS], coloured[NC.SH_DEGREE] = cols, torch.empty(0), 0
    fresh_sh = N.rasterize_gaussians_batch(*other, need_backward=False)[1].cpu().numpy()
    fresh_cols = []
    for v in range(s.V):
        one = NC.one_view(coloured, v)
        one[NC.COLORS] = cols[v].contiguous()
        fresh_cols.append(N.rasterize_gaussians(*one, need_backward=False)[1].cpu().numpy())

    def subject():
        run = _forward(N, s, A, True)
        out = _facts(N, s, run, True, "forward ")
        first, _ = _det(N, s, run, A, "first backward ")
        out.update(first)
        img = _recolor(N, other, run).cpu().numpy()
        assert img.tobytes() == fresh_sh.tobytes(), "recolor at SH degree 2: not the bits of a fresh forward"
        out["sh recolor image"] = img
        out["sh recolor clamped"] = [SS.view_query(N, "CLAMPED", s.P, s.W, s.H, 0, run, v, s.V).cpu().numpy() for v in range(s.V)]
        second, g = _det(N, s, run, A, "sh recolor ", args=other)
        out.update(second)
        img = _recolor(N, s.args, run, colours=cols).cpu().numpy()
        assert img.tobytes() == np.stack(fresh_cols).tobytes(), "colours-per-view recolor: not the bits of fresh forwards"
        out["colour recolor image"] = img
        third, g3 = _det(N, s, run, A, "colour recolor ", args=coloured)
        out.update(third)
        out.update(_followers(N, s, run, "colour recolor ", args=coloured))
        atomic = SS.records_backward(N, coloured, run, s.dpix, False)[0]
        return out, {"atomic": atomic}, {"atomic": g3}

    clean = _hold(N, "recolor_rewrites_saves", s, A, lambda: _donor_training_frame(N, d, A), subject, ("clamped", "records", "final_T"))
    # the three backwards differentiate three different renders
    assert clean["first backward dL_dsh"].tobytes() != clean["sh recolor dL_dsh"].tobytes()
    assert clean["colour recolor dL_dcolor"].any() and not clean["colour recolor dL_dsh"].any()
    assert AC.differing({"m": np.concatenate(clean["forward clamped"])}, {"m": np.concatenate(clean["sh recolor clamped"])}) == ["m"]


def _channels(N, f, A, nx, dev, det):
    """channels-train forward (nx = 8: the split layout) and channels backward on the case's arenas and extra-state block"""
    x, sc, bgx, dx = AC.channel_values(f.pr, f.who, nx, f.V)
    t = lambda a: NC.to_device(a, dev)  # noqa: E731
    extra = (tuple(t(a) for a in x) if isinstance(x, tuple) else t(x), t(sc), t(bgx))
    run = _forward(N, f, A, True, extra=extra, xstate=A.xstate)
    layout = 2 if isinstance(x, tuple) else 0
    g = N.rasterize_gaussians_backward_channels_batch(*NC.channels_backward_args(f.args, run, f.dpix, extra, t(dx)),
                                                      state=(A.xstate, nx, layout), deterministic=det, pairs=CAPACITY[f.pr["name"]])
    gx = g[8]
    gx = torch.cat([gx[0].reshape(-1), gx[1].reshape(-1)]) if isinstance(gx, tuple) else gx
    return run, dict(zip(util.GRAD_NAMES, _np(g[:8])), dL_dextra=gx.cpu().numpy().reshape(-1, 1))


@pytest.mark.parametrize("pair_name", ["main", "deep"])
@pytest.mark.parametrize("direction", ["channels8_then_channels4", "colour_then_channels8"])
def test_channels_state(gpu_device, direction, pair_name):
    """the extra-state block and the arenas between channels frames of eight (split layout) and four channels and colour frames; on
    the deep pair the extras' slice-boundary states are in play"""
    N, pr, dev = _native(), AC.pair(pair_name), gpu_device
    d, s, A = Frame(pr, "D", dev), Frame(pr, "S", dev), Arenas(N, pr, 3, dev)
    nx = 4 if direction == "channels8_then_channels4" else 8

    def donor():
        if direction == "channels8_then_channels4":
            _channels(N, d, A, 8, dev, False)
        else:
            _donor_training_frame(N, d, A)

    def subject():
        run, g = _channels(N, s, A, nx, dev, True)
        out = _facts(N, s, run, True)
        out.update({"channels " + k: x for k, x in g.items()})
        out["channels records"] = _records(N, s, run)
        out.update(_det(N, s, run, A, "colour ")[0])
        _, atomic = _channels(N, s, A, nx, dev, False)
        return out, {"atomic channels": atomic}, {"atomic channels": g}

    # (the extra-state block is written only for quadrants that pass a slice boundary: on the deep pair)
    _hold(N, "channels_state", s, A, donor, subject, ("lists", "records") + (("ckpt",) if pair_name == "deep" else ()) +
          (("xstate",) if pair_name == "deep" and direction == "channels8_then_channels4" else ()))


def test_resume_on_used_binning(gpu_device):
    """the subject at a capacity only some views fit into (the rule of tests/test_gpu_batch_fuzz.py) gets GSR_RETRY, then resumes on
    a larger binning arena the donor filled: the bits of the straight-through call on clean arenas"""
    N, pr, dev = _native(), AC.pair("pingpong"), gpu_device
    d, s, A = Frame(pr, "D", dev), Frame(pr, "S", dev), Arenas(N, pr, 3, dev)
    seen = {}

    def subject():
        if not seen:                     # the clean run: straight through
            run = _forward(N, s, A, True)
            live = sorted(int(x) for x in _facts(N, s, run, True)["list_pairs"])
            assert live[-1] - live[0] >= 2, live
            seen["cap"] = live[0] + (live[-1] - live[0]) // 2
        else:
            tight = torch.zeros((3 * N.lib.gsr_binning_bytes(seen["cap"]),), dtype=torch.uint8, device=dev)
            rc, first = NC.forward_on(N, s.args, A.geom, tight, A.img, True)
            assert rc == 1, "capacity %d: expected GSR_RETRY, got %d" % (seen["cap"], rc)
            rc, run = NC.forward_on(N, s.args, A.geom, A.binning, A.img, True, resume=1, out=(first[1], first[2], None))
            assert rc == 0, N.lib.gsr_last_error()
        out = _facts(N, s, run, True)
        det, g = _det(N, s, run, A)
        out.update(det)
        out.update(_followers(N, s, run))
        return out, {"atomic": _atomic(N, s, run)}, {"atomic": g}

    _hold(N, "resume_on_used_binning", s, A, lambda: _donor_training_frame(N, d, A), subject, ("ranges", "lists", "records"))


def test_stage_pair(gpu_device):
    """gsr_forward_stage1 + gsr_forward_stage2 (one view) on a donor's arenas, then the backward"""
    N, pr, dev = _native(), AC.pair("main"), gpu_device
    d, s, A = Frame(pr, "D", dev, 1), Frame(pr, "S", dev, 1), Arenas(N, pr, 1, dev)

    def subject():
        run = NC.stage_pair_on(N, s.args, A.geom, A.binning, A.img)
        _anchor(N, s, run)
        out = _facts(N, s, run, True)
        det, g = _det(N, s, run, A)
        out.update(det)
        return out, {"atomic": _atomic(N, s, run)}, {"atomic": g}

    _hold(N, "stage_pair", s, A, lambda: _donor_training_frame(N, d, A), subject, ("ranges", "lists", "final_T", "n_contrib", "clamped", "records"))


@pytest.mark.parametrize("pair_name", ["main", "culled"])
def test_nothing_visible(gpu_device, pair_name):
    """views in which every Gaussian is culled, after a full donor: the background, num_rendered 0, every gradient record and
    follower output of the view +0 bits (culled: of the whole batch, every gradient too)"""
    N, pr, dev = _native(), AC.pair(pair_name), gpu_device
    d, s, A = Frame(pr, "D", dev), Frame(pr, "S", dev), Arenas(N, pr, 3, dev)

    def subject():
        run = _forward(N, s, A, True)
        _anchor(N, s, run)
        out = _facts(N, s, run, True)
        det, g = _det(N, s, run, A)
        out.update(det)
        out.update(_followers(N, s, run))
        strict, ws = _contrib(N, s, run)
        out.update(strict)
        out["weight_sum"] = ws["weight_sum"]     # (held by its bits below where it has to be zero)
        return out, {"atomic": _atomic(N, s, run)}, {"atomic": g}

    def donor():
        _donor_training_frame(N, d, A)

    # weight_sum is a float-atomic sum: bitwise only where nothing is visible at all
    def subject_checked():
        out, loose, want = subject()
        if pair_name != "culled":
            ws = out.pop("weight_sum")
            loose, want = dict(loose, contrib={"weight_sum": ws}), dict(want, contrib={"weight_sum": ws})
        return out, loose, want

    clean = _hold(N, "nothing_visible", s, A, donor, subject_checked, ("ranges", "lists", "final_T", "n_contrib", "records"))
    zero = lambda a: not np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8).any()  # noqa: E731
    bg = np.broadcast_to(np.asarray(pr["S"][2], F).reshape(3, 1, 1), (3, s.H, s.W))
    for v in ((2,) if pair_name == "main" else (0, 1, 2)):
        assert clean["num_rendered"][v] == 0 and clean["list_pairs"][v] == 0 and zero(clean["radii"][v])
        assert clean["images"][v].tobytes() == bg.tobytes(), "view %d is not the background" % v
        assert zero(clean["records"][v]) and all(zero(c[v]) for c in clean["cameras"]) and all(zero(x[v]) for x in clean["shares"])
        assert zero(clean["ranges"][v]) and clean["point_list"][v].size == 0
    if pair_name == "culled":
        bad = [(k, clean[k].reshape(-1)[:4]) for k in util.GRAD_NAMES if not zero(clean[k])]
        assert not bad, "gradients of a batch that sees nothing: %s" % bad
        assert all(zero(x) for x in clean["contrib"]) and zero(clean["weight_sum"])
        assert zero(clean["stats"][0]) and zero(clean["stats"][1]) and zero(clean["stats"][2])


def test_depth_sort_ping_pong(gpu_device):
    """the depth sorts of donor and subject run 1, 2, 3 and 2, 3, 4 passes: the subject's order is read from the other buffer than the
    one the donor's sort finished in, in every view"""
    N, pr, dev = _native(), AC.pair("pingpong"), gpu_device
    d, s, A = Frame(pr, "D", dev), Frame(pr, "S", dev), Arenas(N, pr, 3, dev)
    passes = {}

    def words(f, run):
        return [int(SS.view_query(N, "DEPTH_SORT", f.P, f.W, f.H, 0, run, v, f.V)[2]) for v in range(f.V)]

    def donor():
        passes["D"] = words(d, _donor_training_frame(N, d, A))

    def subject():
        run = _forward(N, s, A, True)
        _anchor(N, s, run)
        passes["S"] = words(s, run)
        out = _facts(N, s, run, True)
        det, g = _det(N, s, run, A)
        out.update(det)
        return out, {"atomic": _atomic(N, s, run)}, {"atomic": g}

    _hold(N, "depth_sort_ping_pong", s, A, donor, subject, ("lists", "ranges", "records"))
    assert passes == {"D": [1, 2, 3], "S": [2, 3, 4]}, passes


def test_every_case_has_a_test():
    have = {k[5:] for k in globals() if k.startswith("test_")}
    assert set(AC.CASES) <= have, sorted(set(AC.CASES) - have)
