"""Host check of the footprint clipping and of its row spans (csrc/tile_cull.hpp: clip_rect_to_footprint and the span helpers that
binning.hip's k_duplicate reads the spans back with): tests/footprint_clip_main.cpp is compiled for the host against the very header
the kernels include, and run on seeded random cases against a brute-force walk of the pixels.  What the program draws and what it
counts is described at its top.  The device's v_sqrt_f32, the packing of the spans into a Splat line and the emission itself are
covered by tests/test_gpu_span_edges.py, not here.

The line of this run (CASES, SEED, SPAN_WORDS below; 28 s):
{"cases": 1572864, "misses": 0, "miss_cases": 0, "violations": 0, "decode_mismatches": 0, "nan_degenerate_failures": 0,
"emitted": 11032240, "needed": 9668220, "reference": 34387936, "spans_valid": 1336327, "cut": 437677, "height_8": 20498,
"height_9": 15034, "width_15": 778, "width_16": 191, "too_large": 43517, "off_image": 364687, "ratio_above_8": 166420, "razor":
482847, "razor_inside": 241188, "razor_outside": 241659, "razor_within_3e-4": 318650, "opacity_near_1_255": 524278,
"opacity_below_cut": 89721, "emits_nothing": 193020, "kept_whole": 0, "span_words": 1048576, "span_word_mismatches": 0,
"span_heights": [131451, 130940, 130710, 130894, 130913, 131233, 131256, 131179], "span_empty_first": 231591,
"span_empty_middle": 258588, "span_empty_last": 189495, "span_total_120": 5633, "span_first_14": 127084}

Single-edit mutants of the header, 300 000 cases of seed 1 (misses): the two `fmaxf(.., hx_raw)` extreme-point lines removed 28 977;
`dstar` with the wrong sign 4 926; `pad` = -0.45 (allowance and the strips' half pixel gone) 26 986; `>> 4` replaced by `/ 16` 0 and
the `hyc` clamp dropped 0 -- both reach the cases (4 642 and 1 059 more tiles emitted) but can only widen a span: truncation differs
from the shift below zero alone, where the clamp to the rectangle's first column takes over, and a strip boundary beyond the
ellipse's top or bottom lies on the far side of the extreme point, where the other end of the strip or the extreme point decides."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CASES, SEED, SPAN_WORDS = 3 << 19, 3, 1 << 20


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("footprint_clip") / "footprint_clip")
    # -ffp-contract=off like the library's build (build.py): one rounding per written operation
    subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc"),
                           os.path.join(ROOT, "tests", "footprint_clip_main.cpp"), "-o", exe])
    r = subprocess.run([exe, str(CASES), str(SEED), str(SPAN_WORDS)], capture_output=True, text=True)
    d = json.loads(r.stdout)
    d["returncode"], d["stderr"] = r.returncode, r.stderr
    print(r.stdout)
    return d


def test_the_cases_cover_what_they_should(result):
    d = result
    n = d["cases"]
    assert n >= 1 << 20
    assert d["spans_valid"] >= n // 2
    assert d["cut"] >= n // 6                          # the spans leave out at least one tile of the clipped box
    assert d["height_8"] >= n // 200                   # the encoding's limits: 8 rows (9: no spans) ...
    assert d["width_15"] >= n // 5000                  # ... and 15 columns (16: no spans)
    assert d["height_9"] > 0 and d["width_16"] > 0
    assert d["too_large"] >= n // 100
    assert d["off_image"] >= n // 8                    # the mean left of, right of, above or below the image
    assert d["ratio_above_8"] >= n // 15               # thin footprints (axis ratio after the dilation)
    assert d["razor"] >= n // 8                        # a tile's best pixel placed next to the alpha = 1/255 cut ...
    assert min(d["razor_inside"], d["razor_outside"]) >= 0.4 * d["razor"]      # ... on either side of it ...
    assert d["razor_within_3e-4"] >= n // 16           # ... and close
    assert d["opacity_near_1_255"] >= n // 4 and d["opacity_below_cut"] >= n // 100
    assert 0 < d["emits_nothing"] < n // 2


def test_no_tile_with_a_pixel_that_counts_is_left_out(result):
    assert result["misses"] == 0, result["stderr"]


def test_the_span_bytes_are_well_formed(result):
    assert result["violations"] == 0, result["stderr"]


def test_the_emission_helpers_read_the_spans_back(result):
    d = result
    assert d["decode_mismatches"] == 0 and d["span_word_mismatches"] == 0
    assert d["span_words"] >= 1 << 20
    assert min(d["span_heights"]) >= d["span_words"] // 16          # heights 1-8
    assert min(d["span_empty_first"], d["span_empty_middle"], d["span_empty_last"]) >= d["span_words"] // 16
    assert d["span_total_120"] >= 1000 and d["span_first_14"] >= d["span_words"] // 32


def test_nan_and_degenerate_inputs_keep_the_whole_rectangle(result):
    assert result["nan_degenerate_failures"] == 0, result["stderr"]
    assert result["returncode"] == 0


def test_the_clip_is_tight(result):
    """Tiles emitted against tiles that hold a pixel which counts.  This run: 1.14 (the reference's rectangles: 3.5).  The cap only
    guards against the clip being switched off without anyone noticing."""
    d = result
    print("tiles emitted %d, needed %d, in the reference's rectangles %d" % (d["emitted"], d["needed"], d["reference"]))
    assert d["needed"] <= d["emitted"] <= 1.3 * d["needed"]
    assert d["emitted"] < d["reference"]
