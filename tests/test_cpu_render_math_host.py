"""Host check of the forward kernels' two arithmetic modes (csrc/render_math.hpp): tests/render_math_main.cpp is compiled with g++
against the very header the kernels include and run on seeded random (conic, offset, opacity) draws; what it draws and counts is
described at its top.  The yardstick of the fast form is the EXACT form on the same inputs, both against a float64 evaluation.

The host's exp2f stands in for the device's v_exp_f32 (in both forms): this test pins the algebra and the rounding of everything
around the exponential; the hardware's own exp2 is exercised by tests/test_gpu_render_math.py."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
DRAWS, SEED = 1 << 22, 3
# -ffp-contract=off like the library's build: one rounding per written operation, fusions only where the header writes them
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc"),
         os.path.join(ROOT, "tests", "render_math_main.cpp")]


def _run(exe, draws):
    r = subprocess.run([exe, str(draws), str(SEED)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("render_math") / "render_math")
    subprocess.check_call([CXX] + FLAGS + ["-o", exe])
    return _run(exe, DRAWS)


def test_the_cases_cover_what_they_should(result):
    d = result
    assert d["kept"] >= 2_000_000                                    # alpha in [1/255, 0.99)
    assert d["near_cut"] >= d["kept"] // 50                          # within 5 % of the 1/255 cut
    assert d["on_pixel"] >= d["kept"] // 500                         # the splat centre exactly on the pixel (power = 0)
    assert d["far_pixel"] >= d["kept"] // 4                          # coordinates beyond 3000: few mantissa bits left for the offset
    assert min(d["small_sigma"], d["big_sigma"]) >= d["kept"] // 5   # sub-pixel splats and 10-30 px ones
    assert d["high_rho"] >= d["kept"] // 50                          # |rho| > 0.9


def test_fast_alpha_is_as_accurate_as_the_exact_one(result):
    """Relative error of alpha against float64 over the kept draws.  The bars are ratios to the exact form's own error on the same
    inputs: maximum at most 1.5x, mean at most 2x (a float32 emulation gave 0.82x and 0.9x - 1.25x)."""
    d = result
    print("max relative alpha error: exact %.3g, fast %.3g (%.2fx); mean: exact %.3g, fast %.3g (%.2fx); %d draws kept"
          % (d["max_rel_exact"], d["max_rel_fast"], d["max_rel_fast"] / d["max_rel_exact"], d["mean_rel_exact"], d["mean_rel_fast"],
             d["mean_rel_fast"] / d["mean_rel_exact"], d["kept"]))
    assert 0 < d["max_rel_exact"] < 1e-4 and 0 < d["mean_rel_exact"] < 1e-5     # (the yardstick itself is float32 arithmetic, not garbage)
    assert d["max_rel_fast"] <= 1.5 * d["max_rel_exact"]
    assert d["mean_rel_fast"] <= 2.0 * d["mean_rel_exact"]


def test_the_skips_agree(result):
    """!(p2 > 0) and !(power > 0) take the same side on every kept draw, and a zero-opacity twin yields alpha = 0 in both modes."""
    assert result["sign_disagree"] == 0
    assert result["twin_nonzero"] == 0


def test_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The program is stand-alone (its own main): linked with the sanitizers' runtimes, it needs no preload."""
    exe = str(tmp_path / "render_math_san")
    subprocess.check_call([CXX] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe])
    d = _run(exe, 1 << 18)
    assert d["kept"] > 0 and d["sign_disagree"] == 0 and d["twin_nonzero"] == 0
