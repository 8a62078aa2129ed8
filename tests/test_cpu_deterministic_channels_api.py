"""The deterministic channels backward's boundary, without a GPU: the two C-ABI symbols exist, the scratch-size query behaves, the
new entry refuses every call the channels entry refuses -- same status, same text, compared live in one child process that sees no
device -- and the scratch block's own faults come last; the Python switch (set_deterministic_channels, GSR_DETERMINISTIC_CHANNELS)
opens rasterize_views_channels without touching what set_deterministic does."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import refusal_tables as RT
from refusal_tables import BACKWARD_EXPECTED as EXPECTED, LAYOUT, NX, PAIRS, PKG, PTR, ROT, H, P, W


def test_library_exports_the_deterministic_channels_entries():
    from diff_gaussian_rasterization import _native
    lib = C.CDLL(_native.LIB_PATH)
    for sym in ("gsr_backward_batch_channels_det", "gsr_backward_det_channels_bytes"):
        assert hasattr(lib, sym), "libgsr_hip.so does not export %s" % sym
        assert sym in _native.SYMBOLS
    assert "backward_channels_det" in _native.CALLS


def test_scratch_size_query():
    from diff_gaussian_rasterization import _native
    f, colour = _native.lib.gsr_backward_det_channels_bytes, _native.lib.gsr_backward_det_bytes
    W_, H_, P_ = 1920, 1080, 800_000
    for nx, layout in ((4, 0), (4, 1), (8, 0), (8, 1), (8, 2)):
        prev = 0
        for pairs in (0, 1, 4095, 4096, 4097, 100_000, 1_100_000, 7_300_000, 87_000_000):
            b = f(1, P_, W_, H_, pairs, nx, layout)
            assert b % 256 == 0 and b >= prev and b >= colour(1, P_, W_, H_, pairs), (nx, layout, pairs, b, prev)
            prev = b
        assert f(1, P_, W_, H_, 7_300_000, nx, layout) > f(1, P_, W_, H_, 1_100_000, nx, layout) > f(1, P_, W_, H_, 0, nx, layout)
        for V in (2, 3, 12):
            assert f(V, P_, W_, H_, 1_100_000, nx, layout) > f(V - 1, P_, W_, H_, 1_100_000, nx, layout)
            assert f(V, P_, W_, H_, 1_100_000, nx, layout) >= colour(V, P_, W_, H_, 1_100_000)
        # the extras' slots: 16 nx bytes per pair and view on top of the colour block
        extra = f(1, 0, W_, H_, 7_300_000, nx, layout) - colour(1, 0, W_, H_, 7_300_000)
        assert 16 * nx * 7_300_000 <= extra < 16 * nx * 7_300_000 + 4096
    for layout in (0, 1):
        assert f(2, P_, W_, H_, 1_100_000, 8, layout) > f(2, P_, W_, H_, 1_100_000, 4, layout)
    # the staging of the rows the views share follows P: 4 V P nx bytes (layout 0), 16 V P bytes (layout 2), nothing (layout 1)
    for nx, layout, per in ((4, 0, 16), (8, 0, 32), (8, 2, 16), (4, 1, 0), (8, 1, 0)):
        d = f(3, P_, W_, H_, 1000, nx, layout) - f(3, 0, W_, H_, 1000, nx, layout)
        assert per * 3 * P_ <= d < per * 3 * P_ + 256, (nx, layout, d)
    assert f(1, 0, 16, 16, 0, 4, 0) > 0                                # P = 0, no pairs: still a valid (small) block
    # nonsense shapes, and what the channels forward refuses: no size
    assert f(0, P_, W_, H_, 10, 8, 0) == 0 and f(-1, P_, W_, H_, 10, 8, 0) == 0
    assert f(1, P_, 0, H_, 10, 8, 0) == 0 and f(1, P_, -4, H_, 10, 8, 0) == 0 and f(1, P_, W_, 0, 10, 8, 0) == 0
    for nx in (0, 1, 3, 5, 7, 9, 12, 16, -4):
        assert f(1, P_, W_, H_, 10, nx, 0) == 0, nx
    assert f(1, P_, W_, H_, 10, 4, 2) == 0
    assert f(1, P_, W_, H_, 10, 8, 3) == 0 and f(1, P_, W_, H_, 10, 8, -1) == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _run_table():
    """(child process, no device) -> {"rows": {case: [[rc, text] of gsr_backward_batch_channels, [rc, text] of the new entry]},
    "scratch": {case: [rc, text]}, "sizes": {...}}"""
    N = RT.native_without_device()
    lib = N.lib
    frame = lambda name: RT.frame(N, name)  # noqa: E731

    def call(fr, kw, which):
        """which: 'channels', or 'det' (the new entry; scratch / scratch_bytes from kw, default a dummy pointer of 0 bytes)"""
        kw = dict(kw)
        a = fr
        c = dict(a, V=1, radii=PTR, dpix=PTR, dmean2D=PTR, dopacity=PTR, dcolor=PTR, dmean3D=PTR, dcov3D=PTR, dsh=PTR, dscale=PTR,
                 drot=ROT, scratch=PTR, scratch_bytes=0, nx=NX, layout=LAYOUT, extra=PTR, bg_extra=PTR, dextra=PTR, dvalues=PTR,
                 params=True)
        pk = {k: kw.pop(k) for k in list(kw) if k in ("P", "W", "H", "M", "means3D", "shs", "colors_precomp", "scales", "rotations")}
        if "binning_pairs" in kw:
            c["binning_bytes"] = lib.gsr_binning_bytes(kw.pop("binning_pairs"))
        c.update(kw)
        p = RT.params(N, **pk)
        args = [C.byref(p) if c["params"] else None, c["V"], c["radii"], c["geom"], c["geom_bytes"], c["binning"], c["binning_bytes"],
                c["image"], c["image_bytes"], c["dpix"], c["dmean2D"], c["dopacity"], c["dcolor"], c["dmean3D"], c["dcov3D"], c["dsh"],
                c["dscale"], c["drot"], c["nx"], c["layout"], c["extra"], None, c["bg_extra"], c["state"], c["state_bytes"],
                c["dextra"], c["dvalues"]]
        if which == "channels":
            rc = lib.gsr_backward_batch_channels(*args, None)
        else:
            rc = lib.gsr_backward_batch_channels_det(*args, c["scratch"], c["scratch_bytes"], None)
        return [rc, lib.gsr_last_error().decode() if rc != 0 else ""]

    rows = {}
    for entry, case, fr, kw in RT.backward_table():
        if entry != "channels":
            continue
        a = frame(fr)
        if kw.get("state") == "other":
            kw = dict(kw, state=RT.buf(16))
        rows[case] = [call(a, kw, "channels"), call(a, kw, "det")]

    # the scratch block's own faults, on arenas every other check passes
    scratch = {}
    good = frame("chan_train")
    scratch["null"] = call(good, dict(scratch=None, scratch_bytes=1 << 30), "det")
    m = re.search(r"< (\d+) = gsr_backward_det_channels_bytes\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", scratch["null"][1])
    need, qargs = (int(m.group(1)), [int(g) for g in m.groups()[1:]]) if m else (0, [1, P, W, H, PAIRS, NX, LAYOUT])
    query = int(lib.gsr_backward_det_channels_bytes(*qargs))
    colour = int(lib.gsr_backward_det_bytes(*qargs[:5]))
    scratch["one_byte_short"] = call(good, dict(scratch_bytes=query - 1), "det")
    scratch["colour_sized"] = call(good, dict(scratch_bytes=colour), "det")
    scratch["zero_bytes"] = call(good, dict(), "det")
    good2 = frame("chan_train_v2")
    scratch["two_views"] = call(good2, dict(V=2, scratch_bytes=100000), "det")
    # a scratch fault next to another fault: the other one wins, with the channels entry's text
    both = {}
    for name, fr, kw in (("record_colour_forward", "fwd_nb1", {}), ("record_none", "none", {}), ("record_other_nx", "chan_train", dict(nx=4)),
                         ("pointer", "chan_train", dict(radii=None)), ("state_too_small_for_binning", "chan_train", dict(binning_pairs=100000)),
                         ("geom_too_small", "chan_train", dict(geom_bytes=100))):
        a = frame(fr)
        both[name] = [call(a, kw, "channels"), call(a, dict(kw, scratch=None, scratch_bytes=0), "det")]
    return dict(rows=rows, scratch=scratch, both=both, sizes=dict(need=need, query=query, colour=colour, qargs=qargs))


@pytest.fixture(scope="module")
def refusals():
    return RT.child_json(__file__)


def test_every_channels_refusal_is_the_new_entrys_too(refusals):
    rows = refusals["rows"]
    want = sorted(k[len("channels/"):] for k in EXPECTED if k.startswith("channels/"))
    assert len(want) >= 40 and sorted(rows) == want                    # every case of the existing channels rows
    wrong = {k: v for k, v in rows.items() if v[0] != v[1] or v[0][0] == 0}
    assert not wrong, "\n".join("%s: gsr_backward_batch_channels %r, gsr_backward_batch_channels_det %r" % (k, a, b)
                                for k, (a, b) in wrong.items())


def test_channels_entry_still_refuses_as_pinned(refusals):
    """(the live comparison above compares against THIS build's channels entry: it still answers with the committed literals)"""
    for k, (a, _) in refusals["rows"].items():
        assert tuple(a) == EXPECTED["channels/" + k], k


@pytest.mark.parametrize("case", ["null", "one_byte_short", "colour_sized", "zero_bytes", "two_views"])
def test_scratch_faults_are_capacity_errors_that_name_the_needed_size(refusals, case):
    from diff_gaussian_rasterization import _native
    s = refusals["sizes"]
    assert s["need"] == s["query"] > s["colour"] > 0                   # the message's size is the size query's, for the arguments it names
    assert s["qargs"][:4] == [1, P, W, H] and s["qargs"][5:] == [NX, LAYOUT]
    rc, text = refusals["scratch"][case]
    assert rc == -3, (rc, text)                                        # GSR_ERR_CAPACITY
    m = re.search(r"< (\d+) = gsr_backward_det_channels_bytes\(([-\d, ]+)\)", text)
    assert m, text
    args = [int(t) for t in m.group(2).split(",")]
    assert int(m.group(1)) == _native.lib.gsr_backward_det_channels_bytes(*args), text
    assert args[0] == (2 if case == "two_views" else 1)


def test_any_other_fault_wins_over_a_scratch_fault(refusals):
    for name, (chan, det) in refusals["both"].items():
        assert chan[0] != 0 and det == chan, (name, chan, det)
        assert "scratch" not in det[1], (name, det)


# ---- the Python switch --------------------------------------------------------------------------------------------------------
def _call(d):
    z = torch.zeros((4, 3))
    return d.rasterize_views_channels(z, z, torch.zeros((4, 1)), [object()], torch.zeros((4, 4)), torch.zeros(4), shs=None,
                                      colors_precomp=z, scales=z, rotations=torch.zeros((4, 4)))


def test_switch_is_off_by_default_and_exported():
    import diff_gaussian_rasterization as d
    e = dict(os.environ)
    e.pop("GSR_DETERMINISTIC_CHANNELS", None)
    e["PYTHONPATH"] = PKG + os.pathsep + e.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", "import diff_gaussian_rasterization as d; print(d.get_deterministic_channels())"],
                         env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "False"
    was = d.get_deterministic_channels()
    try:
        for v in (True, False, 1, 0):
            d.set_deterministic_channels(v)
            assert d.get_deterministic_channels() is bool(v)
    finally:
        d.set_deterministic_channels(was)


@pytest.mark.parametrize("env,want", [("1", "True"), ("0", "False"), ("", "False")])
def test_environment_sets_the_initial_value(env, want):
    e = dict(os.environ)
    e["GSR_DETERMINISTIC_CHANNELS"] = env
    e["PYTHONPATH"] = PKG + os.pathsep + e.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", "import diff_gaussian_rasterization as d; print(d.get_deterministic_channels(), d.get_deterministic())"],
                         env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == want + " None"       # (the colour backward's switch is not touched)


def test_switch_opens_the_channels_call_and_closing_it_restores_the_refusal():
    """(everything here happens before anything touches a device)"""
    import diff_gaussian_rasterization as d
    was, was_x, torch_was = d.get_deterministic(), d.get_deterministic_channels(), torch.are_deterministic_algorithms_enabled()
    warn_was = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        d.set_deterministic_channels(False)
        d.set_deterministic(True)
        with pytest.raises(RuntimeError, match="no deterministic backward") as ei:
            _call(d)
        assert "set_deterministic_channels" in str(ei.value)           # the refusal points at the new switch
        d.set_deterministic_channels(True)
        with pytest.raises(Exception) as ei:                           # past the switch: fails later, on the dummy settings object
            _call(d)
        assert "no deterministic backward" not in str(ei.value)
        assert d.get_deterministic() is True                           # (the other switch is left alone)
        d.set_deterministic(None)
        torch.use_deterministic_algorithms(True)
        with pytest.raises(Exception) as ei:
            _call(d)
        assert "no deterministic backward" not in str(ei.value)
        d.set_deterministic_channels(False)
        with pytest.raises(RuntimeError, match="no deterministic backward"):
            _call(d)
        d.set_deterministic(True)
        torch.use_deterministic_algorithms(False)
        with pytest.raises(RuntimeError, match="no deterministic backward"):
            _call(d)
    finally:
        torch.use_deterministic_algorithms(torch_was, warn_only=warn_was)
        d.set_deterministic(was)
        d.set_deterministic_channels(was_x)


def test_binding_takes_the_new_keywords():
    import inspect
    from diff_gaussian_rasterization import _native
    ps = inspect.signature(_native.rasterize_gaussians_backward_channels_batch).parameters
    assert ps["deterministic"].default is False and ps["pairs"].default is None
    assert list(ps)[-4:-1] == ["state", "deterministic", "pairs"]


if __name__ == "__main__":
    print(json.dumps(_run_table()))
