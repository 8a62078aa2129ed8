"""The deterministic colour backward's boundary, without a GPU: the two C-ABI symbols exist, the scratch-size query behaves, and
the Python switch follows its rules (default None = torch's deterministic-algorithms flag, explicit values, GSR_DETERMINISTIC)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-pcloud-render_amd")


def test_library_exports_the_deterministic_entries():
    from diff_gaussian_rasterization import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for sym in ("gsr_backward_batch_det", "gsr_backward_det_bytes"):
        assert hasattr(lib, sym), "libgsr_hip.so does not export %s" % sym
        assert sym in _native.SYMBOLS


def test_scratch_size_query():
    from diff_gaussian_rasterization import _native
    f = _native.lib.gsr_backward_det_bytes
    W, H, P = 1920, 1080, 800_000
    assert f(1, 0, W, H, 0) > 0 and f(1, 0, 16, 16, 0) > 0            # P = 0, no pairs: still a valid (small) block
    prev = 0
    for pairs in (0, 1, 4095, 4096, 4097, 100_000, 1_100_000, 7_300_000, 87_000_000):
        b = f(1, P, W, H, pairs)
        assert b % 256 == 0 and b >= prev, (pairs, b, prev)
        prev = b
    assert f(1, P, W, H, 7_300_000) > f(1, P, W, H, 1_100_000) > f(1, P, W, H, 0)
    one = f(1, P, W, H, 1_100_000)
    for V in (2, 3, 12):
        b = f(V, P, W, H, 1_100_000)
        assert b % 256 == 0 and b > f(V - 1, P, W, H, 1_100_000)
        assert b == V * (one - 256) + 256                             # V identically laid out per-view blocks
    # a 64-B slot per quadrant (256 B), the sort's four u32 buffers (16 B) and a flag word (4 B) per pair, plus the sort's histograms
    assert 276 * 7_300_000 <= f(1, P, W, H, 7_300_000) < 278 * 7_300_000
    # the figure the header states for the headline workload: 12 views of 7.3 M pairs
    assert 24.0e9 < f(12, P, W, H, 7_300_000) < 24.5e9
    assert f(0, P, W, H, 10) == 0 and f(1, P, 0, H, 10) == 0          # nonsense shapes: no size


def test_switch_defaults_and_explicit_values():
    import diff_gaussian_rasterization as d
    from diff_gaussian_rasterization import _native
    was = d.get_deterministic()
    try:
        d.set_deterministic(None)
        assert d.get_deterministic() is None
        for v in (True, False, None, 1, 0):
            d.set_deterministic(v)
            assert d.get_deterministic() is (None if v is None else bool(v))
            if v is not None:
                assert _native.deterministic_active() is bool(v)
    finally:
        d.set_deterministic(was)


def test_switch_follows_torch_when_unset():
    import diff_gaussian_rasterization as d
    from diff_gaussian_rasterization import _native
    was, torch_was = d.get_deterministic(), torch.are_deterministic_algorithms_enabled()
    warn_was = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        d.set_deterministic(None)
        torch.use_deterministic_algorithms(False)
        assert _native.deterministic_active() is False
        torch.use_deterministic_algorithms(True)
        assert _native.deterministic_active() is True
        d.set_deterministic(False)                                    # an explicit value wins over torch's flag
        assert _native.deterministic_active() is False
        torch.use_deterministic_algorithms(False)
        d.set_deterministic(True)
        assert _native.deterministic_active() is True
    finally:
        torch.use_deterministic_algorithms(torch_was, warn_only=warn_was)
        d.set_deterministic(was)


@pytest.mark.parametrize("env,want", [(None, "None"), ("0", "False"), ("1", "True"), ("", "None")])
def test_environment_sets_the_initial_value(env, want):
    e = dict(os.environ)
    e.pop("GSR_DETERMINISTIC", None)
    if env is not None:
        e["GSR_DETERMINISTIC"] = env
    e["PYTHONPATH"] = PKG + os.pathsep + e.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", "import diff_gaussian_rasterization as d; print(d.get_deterministic())"],
                         env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == want


def test_channels_call_is_refused_when_the_path_is_forced_on():
    """(raised before anything touches a device)"""
    import diff_gaussian_rasterization as d
    was = d.get_deterministic()
    z = torch.zeros((4, 3))
    try:
        d.set_deterministic(True)
        with pytest.raises(RuntimeError, match="no deterministic backward"):
            d.rasterize_views_channels(z, z, torch.zeros((4, 1)), [object()], torch.zeros((4, 4)), torch.zeros(4), shs=None,
                                       colors_precomp=z, scales=z, rotations=torch.zeros((4, 4)))
    finally:
        d.set_deterministic(was)


def test_channels_call_follows_torch_convention_when_unset():
    import diff_gaussian_rasterization as d
    was, torch_was = d.get_deterministic(), torch.are_deterministic_algorithms_enabled()
    warn_was = torch.is_deterministic_algorithms_warn_only_enabled()
    z = torch.zeros((4, 3))

    def call():
        return d.rasterize_views_channels(z, z, torch.zeros((4, 1)), [object()], torch.zeros((4, 4)), torch.zeros(4), shs=None,
                                          colors_precomp=z, scales=z, rotations=torch.zeros((4, 4)))
    try:
        d.set_deterministic(None)
        torch.use_deterministic_algorithms(True)
        with pytest.raises(RuntimeError, match="no deterministic backward"):
            call()
        torch.use_deterministic_algorithms(True, warn_only=True)
        with pytest.warns(UserWarning, match="no deterministic backward"):
            with pytest.raises(Exception) as ei:       # past the switch: the call goes on and fails on the dummy settings object
                call()
        assert "no deterministic backward" not in str(ei.value)
    finally:
        torch.use_deterministic_algorithms(torch_was, warn_only=warn_was)
        d.set_deterministic(was)
