"""The switch of the training calls' arithmetic (include/gsr.h gsr_set_train_math; GSR_TRAIN_MATH), without a GPU: the symbol, query /
set / refuse, its independence of gsr_set_render_math, the Python setter's two spellings and the environment's initial value.  What
the mode computes is tests/test_cpu_train_math_host.py (host arithmetic) and tests/test_gpu_train_math.py (the kernels)."""
import os
import subprocess
import sys

import pytest

import util  # noqa: F401  (puts the package on sys.path)

PKG = util.PKG


def test_the_library_exports_the_symbol():
    from diff_gaussian_rasterization import _native as N
    assert "gsr_set_train_math" in N.SYMBOLS
    assert "gsr_set_train_math" in N._DECL
    getattr(N.lib, "gsr_set_train_math")
    with open(os.path.join(util.ROOT, "include", "gsr.h")) as f:
        assert "int gsr_set_train_math(int mode);" in f.read()


def test_query_set_and_refusal():
    from diff_gaussian_rasterization import _native as N
    f = N.lib.gsr_set_train_math
    was = f(-1)
    try:
        assert was in (0, 1)
        assert f(1) == 1 and f(-1) == 1
        assert f(-7) == 1                      # any negative value only queries
        for bad in (2, 3, 255, 1 << 20):       # refused: the value in force is returned unchanged
            assert f(bad) == 1 and f(-1) == 1
        assert f(0) == 0 and f(-1) == 0
        for bad in (2, 17):
            assert f(bad) == 0 and f(-1) == 0
    finally:
        f(was)


def test_the_two_switches_do_not_move_each_other():
    from diff_gaussian_rasterization import _native as N
    train, render = N.lib.gsr_set_train_math, N.lib.gsr_set_render_math
    was_t, was_r = train(-1), render(-1)
    try:
        for r in (0, 1):
            assert render(r) == r
            for t in (0, 1, 0):
                assert train(t) == t and render(-1) == r
                assert train(2) == t and render(-1) == r       # a refused value moves neither
        for t in (0, 1):
            assert train(t) == t
            for r in (0, 1, 0):
                assert render(r) == r and train(-1) == t
                assert render(2) == r and train(-1) == t
    finally:
        train(was_t)
        render(was_r)


def test_python_setter_accepts_both_spellings():
    import diff_gaussian_rasterization as d
    from diff_gaussian_rasterization import _native as N
    was, was_r = d.get_train_math(), d.get_render_math()
    try:
        assert was in ("exact", "fast")
        assert d.set_train_math("fast") == "fast" and d.get_train_math() == "fast" and N.lib.gsr_set_train_math(-1) == 1
        assert d.set_train_math(0) == "exact" and d.get_train_math() == "exact" and N.lib.gsr_set_train_math(-1) == 0
        assert d.set_train_math(1) == "fast" and d.get_train_math() == "fast"
        assert d.set_train_math("exact") == "exact" and d.get_train_math() == "exact"
        for bad in ("quick", 2, -1, True, None):
            with pytest.raises((ValueError, TypeError)):
                d.set_train_math(bad)
            assert d.get_train_math() == "exact"
        assert d.get_render_math() == was_r
    finally:
        d.set_train_math(was)


@pytest.mark.parametrize("env,want", [(None, "exact"), ("0", "exact"), ("1", "fast")])
def test_environment_sets_the_initial_value(env, want):
    e = dict(os.environ)
    e.pop("GSR_TRAIN_MATH", None)
    e.pop("GSR_RENDER_MATH", None)
    if env is not None:
        e["GSR_TRAIN_MATH"] = env
    e["PYTHONPATH"] = PKG + os.pathsep + e.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", "import diff_gaussian_rasterization as d; print(d.get_train_math(), d.get_render_math())"],
                         env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == want + " exact"     # (and the environment of one switch leaves the other alone)
