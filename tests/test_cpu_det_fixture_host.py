"""Host check of the fixture behind the ordered reductions' self-tests (csrc/det_fixture.hpp): tests/det_fixture_main.cpp is compiled
with g++ against the very header det_backward.hip includes, under the address and undefined-behaviour sanitizers, and run.  What it
checks is described at its top: the forced run lengths, the run without a mark, Gaussians without a run, and the reference sum at the
three slot widths against a sum written another way.  The device side of the same fixture runs in N.selftest (GPU tests)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


def test_fixture_and_reference_sum_under_sanitizers(tmp_path):
    """The program is stand-alone (its own main): linked with the sanitizers' runtimes, it needs no preload."""
    exe = str(tmp_path / "det_fixture_san")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc"),
                           os.path.join(ROOT, "tests", "det_fixture_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(r.stdout)
    assert d["failed"] == 0 and d["runs"] > 11 and d["without_run"] > 0
