"""Host check of what the fast render backward adds to csrc/render_math.hpp (gsr_set_train_math): tests/train_math_main.cpp is compiled
with g++ against the very header the kernels include and run on the seeded draws of tests/render_math_main.cpp (sigma 0.3 - 30 px,
|rho| <= 0.95, coordinates to 4000).

  (a) the G / alpha form the backward evaluates (alpha_fast_g) gives alpha_fast(o, p2) bit for bit on every draw, G = 2^p2 bit for
      bit, and the same hit decision -- so the fast backward takes the decisions of the fast forward that wrote n_contrib;
  (b) the flush's unfolding of the staged (folded) conic returns the conic within 3e-7 relative: four roundings of 2^-24, two
      products and two rounded constants (4 x 5.96e-8 = 2.4e-7).

The host's exp2f stands in for the device's v_exp_f32 in both forms; the hardware's exp2 is exercised by tests/test_gpu_train_math.py."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
DRAWS, SEED = 1 << 22, 3
UNFOLD_REL = 3e-7
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc"),
         os.path.join(ROOT, "tests", "train_math_main.cpp")]


def _run(exe, draws):
    r = subprocess.run([exe, str(draws), str(SEED)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("train_math") / "train_math")
    subprocess.check_call([CXX] + FLAGS + ["-o", exe])
    return _run(exe, DRAWS)


def test_the_draws_fall_on_both_sides_of_every_decision(result):
    d = result
    assert d["used"] >= 3_000_000
    assert d["hits"] >= d["used"] // 4 and d["misses_alpha"] >= d["used"] // 20      # alpha on either side of 1/255
    assert d["near_cut"] >= d["used"] // 50                                          # within 5 % of the cut
    assert d["clamped"] >= 100                                                       # min(0.99, .) taken


def test_backward_alpha_is_the_forward_alpha_bit_for_bit(result):
    d = result
    assert d["alpha_differs"] == 0 and d["g_differs"] == 0 and d["hit_differs"] == 0


def test_unfolding_returns_the_conic(result):
    d = result
    print("unfold(fold(x)): max relative error %.3g (bar %.1e)" % (d["max_unfold_rel"], UNFOLD_REL))
    assert d["twice_inexact"] == 0
    assert 0 < d["max_unfold_rel"] <= UNFOLD_REL


def test_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The program is stand-alone (its own main): linked with the sanitizers' runtimes, it needs no preload."""
    exe = str(tmp_path / "train_math_san")
    subprocess.check_call([CXX] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe])
    d = _run(exe, 1 << 18)
    assert d["used"] > 0 and d["alpha_differs"] == 0 and d["hit_differs"] == 0 and d["max_unfold_rel"] <= UNFOLD_REL
