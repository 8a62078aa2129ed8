"""Host check of the footprint test's algebra (csrc/tile_cull.hpp: may_touch_rect): tests/footprint_bound_main.cpp is compiled for
the host against the very header the kernels include, and run on seeded random cases.  What the program draws and what it counts
is described at its top.  The device's v_rcp_f32 / v_log_f32 are covered by the GPU tests, not here."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CASES, SEED = 1 << 22, 2


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("footprint_bound") / "footprint_bound")
    # -ffp-contract=off like the library's build (build.py): one rounding per written operation
    subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc"),
                           os.path.join(ROOT, "tests", "footprint_bound_main.cpp"), "-o", exe])
    r = subprocess.run([exe, str(CASES), str(SEED)], capture_output=True, text=True)
    d = json.loads(r.stdout)
    d["returncode"], d["stderr"] = r.returncode, r.stderr
    print(r.stdout)
    return d


def test_the_cases_cover_what_they_should(result):
    d = result
    assert d["cases"] >= 1 << 20
    assert min(d["regions"]) >= d["cases"] // 10                     # all nine positions of the centre around the rectangle
    assert d["rho_above_0.99"] >= d["cases"] // 10                   # strongly correlated conics
    assert min(d["one_pixel"], d["one_row"], d["one_column"]) >= d["cases"] // 20
    assert d["opacity_near_1_255"] >= d["cases"] // 4
    assert d["razor_edge"] >= d["cases"] // 8                        # best pixel within +-0.2 % of the 1/255 threshold
    # neither answer is the trivial one
    assert d["cases"] // 4 <= d["counted"] <= d["kept_new"] <= 3 * d["cases"] // 4


def test_no_entry_that_counts_at_some_pixel_is_dropped(result):
    assert result["misses"] == 0, result["stderr"]


def test_price_against_the_four_edge_form(result):
    """Cases the two-edge bound with the log2 threshold keeps and the four-edge form with logf drops.  Measured over 8 seeds x 4 194 304
    cases: 8 of 33 554 432 (2.4e-7; 7 the other way round -- the two differ only by the rounding of the threshold); this run's own
    figure (seed 2) is 2 of 4 194 304.  The cap is twice that."""
    print("kept by the new bound only: %d, by the four-edge form only: %d, of %d" % (result["new_not_4edge"], result["4edge_not_new"], result["cases"]))
    assert result["new_not_4edge"] <= 4


def test_nan_inputs_keep(result):
    assert result["nan_drops"] == 0
    assert result["returncode"] == 0
