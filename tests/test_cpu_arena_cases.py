"""The inputs of tests/test_gpu_arena_state.py, held to what that test needs from them -- from the oracle alone, without the library:
the donor frames really leave behind what the subject frames must not see (tests/arena_cases.py census), the comparison really
reports a flipped bit, and every row of DESIGN.md's arena-contract table names a case that exists."""
import os
import re

import numpy as np
import pytest

import arena_cases as AC
import util
from oracle.oracle import Oracle


@pytest.fixture(scope="module")
def census():
    oracle = Oracle()
    return {name: AC.census(AC.pair(name), oracle) for name in AC.PAIRS}


def test_pairs_share_what_carves_the_arenas():
    for name in AC.PAIRS:
        pr = AC.pair(name)
        d, s = AC.scenes(pr, "D"), AC.scenes(pr, "S")
        assert len(d) == len(s) == pr["V"] == 3
        assert AC.P % 256 != 0 and AC.P % 64 != 0
        for a, b in zip(d, s):
            assert (a.P, a.W, a.H, a.M, a.tanfovx, a.tanfovy) == (b.P, b.W, b.H, b.M, b.tanfovx, b.tanfovy) == \
                (AC.P, pr["W"], pr["H"], AC.SH_ROWS, a.tanfovx, a.tanfovy), name
            assert a.sh_degree != b.sh_degree and not np.array_equal(a.means3D, b.means3D) and not np.array_equal(a.shs, b.shs)
            assert not np.array_equal(a.viewmatrix, b.viewmatrix) and not np.array_equal(a.bg, b.bg), name


def test_tiles_empty_out_and_fill_up(census):
    """every pair, every view the GPU cases compare (a view in which S sees nothing holds it trivially and is asserted too)"""
    for name in AC.PAIRS:
        for v, c in enumerate(census[name]):
            assert 5 * c["d_only"] >= c["tiles"], "%s view %d: %d of %d tiles have a list in D and none in S" % (name, v, c["d_only"], c["tiles"])
    assert any(c["s_only"] > 0 for c in census["main"]), "no tile is empty in D and filled in S"


def test_a_view_and_a_whole_batch_see_nothing(census):
    last = census["main"][2]
    assert last["pairs_s"] == 0 and last["visible_s"] == 0 and last["pairs_d"] > 0 and last["visible_d"] == AC.P
    assert all(c["pairs_s"] > 0 for c in census["main"][:2])
    assert all(c["pairs_s"] == 0 and c["visible_s"] == 0 and c["pairs_d"] > 0 for c in census["culled"])


def test_the_donor_leaves_a_longer_list_behind(census):
    for name in AC.PAIRS:
        for v, c in enumerate(census[name]):
            assert c["pairs_d"] > c["pairs_s"], (name, v, c["pairs_d"], c["pairs_s"])


def test_visibility_and_clamp_masks_differ(census):
    for name in ("main", "pingpong", "deep"):
        for v, c in enumerate(census[name]):
            if c["pairs_s"] == 0:
                continue
            assert 100 * c["clamp_differs"] >= c["both"] > 0, (name, v, c["clamp_differs"], c["both"])
    for name in AC.PAIRS:
        for v, c in enumerate(census[name]):
            assert 20 * c["visible_d_only"] >= AC.P, (name, v, c["visible_d_only"])


def test_depth_sorts_end_in_different_buffers(census):
    c = census["pingpong"]
    assert [x["passes_d"] for x in c] == [1, 2, 3] and [x["passes_s"] for x in c] == [2, 3, 4]
    assert all((x["passes_d"] ^ x["passes_s"]) & 1 for x in c)


def test_slice_boundaries_are_crossed_in_different_quadrants(census):
    """at both slice lengths (512 entries at V = 1, 1024 from V = 2), in every view: quadrants whose walk passes a boundary in D and
    cannot in S, and the other way round"""
    for v, c in enumerate(census["deep"]):
        assert c["longest_d"] > 1024 and c["longest_s"] > 1024
        for L in AC.SLICES:
            assert c["cross_d_only"][L] > 0 and c["cross_s_only"][L] > 0, (v, L, c)
    # ... and the other pairs stay inside one slice, so that what they find is not the boundary states'
    for name in ("main", "pingpong"):
        assert all(max(c["longest_d"], c["longest_s"]) < 512 for c in census[name]), name


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def _sample():
    rng = np.random.default_rng(5)
    return AC.outputs(images=rng.uniform(0, 1, (2, 3, 4, 5)).astype(np.float32), radii=rng.integers(0, 9, (2, 7)).astype(np.int32),
                      num_rendered=np.array([5, 0], np.int64), clamped=[rng.integers(0, 2, (7, 3)).astype(np.uint8) for _ in range(2)],
                      grads=[rng.normal(0, 1, (7, 3)).astype(np.float32), np.array([np.nan, 0.0, -0.0], np.float32)], absent=None)


def test_outputs_names_every_array():
    assert sorted(_sample()) == ["clamped[0]", "clamped[1]", "grads[0]", "grads[1]", "images", "num_rendered", "radii"]


def test_differing_reports_one_flipped_bit_in_every_kind_of_output():
    a = _sample()
    assert AC.differing(a, _sample()) == []            # (equal NaN payloads are equal)
    for k in a:
        b = _sample()
        w = b[k].reshape(-1).view(np.uint8)
        w[w.size // 2 // b[k].itemsize * b[k].itemsize] ^= 1    # the low bit of one element (little endian)
        assert AC.differing(a, b) == [k] == AC.differing(b, a), k


def test_differing_tells_zero_signs_and_nan_payloads_apart():
    a, b = _sample(), _sample()
    b["grads[1]"][1] = -0.0
    assert AC.differing(a, b) == ["grads[1]"]
    b = _sample()
    b["grads[1]"].view(np.uint32)[0] ^= 1               # another NaN
    assert AC.differing(a, b) == ["grads[1]"]


def test_differing_reports_shapes_types_and_missing_names():
    a = _sample()
    b = _sample()
    b["images"] = b["images"].reshape(2, 3, 20)
    assert AC.differing(a, b) == ["images"]
    b = _sample()
    b["radii"] = b["radii"].view(np.uint32)
    assert AC.differing(a, b) == ["radii"]
    b = _sample()
    del b["num_rendered"]
    assert AC.differing(a, b) == ["num_rendered"] == AC.differing(b, a)
    b = _sample()
    b["radii"] = b["radii"][:, :6]
    assert AC.differing(a, b) == ["radii"]


# ---- the layout the positive control relies on -------------------------------------------------------------------------------------
def test_the_boundary_states_lie_where_ckpt_region_looks():
    """native_calls.ckpt_region restates csrc/common.hpp: the slice-boundary states are the LAST array bin_view carves, one slot of
    256 float4 per BWD_CHUNK_SHIFT_MIN-entry slice of the capacity plus two.  Held to the header's text, so that a change of the
    layout fails here instead of pointing the positive control at other bytes"""
    import native_calls as NC
    text = open(os.path.join(util.PKG, "csrc", "common.hpp")).read()
    assert int(re.search(r"constexpr int BWD_CHUNK_SHIFT_MIN = (\d+);", text).group(1)) == NC.CKPT_SHIFT
    body = text[text.index("inline BinView bin_view("):text.index("// largest capacity whose arena fits")]
    carves = re.findall(r"carve\(cur, b\.(\w+(?:\[\d\])?), (.+)\);", body)
    assert [c[0] for c in carves] == ["key[0]", "key[1]", "val[0]", "val[1]", "hist", "totals", "ckpt"], carves
    assert carves[-1][1] == "((r >> BWD_CHUNK_SHIFT_MIN) + 2) * 256"
    assert re.search(r"float4\* ckpt;", text[text.index("struct BinView"):text.index("struct ImageView")])
    assert NC.CKPT_SLOT_BYTES == 256 * 16                                    # 256 float4 per slot
    assert "b.bytes = (size_t)(cur - reinterpret_cast<char*>(base));" in body and "align_up(count * sizeof(T), 256)" in text
    # a view's share of the allocation and its capacity: api.hip make_batch
    api = open(os.path.join(util.PKG, "csrc", "api.hip")).read()
    assert "const size_t per_view = ((binning_bytes - 256) / (size_t)V) / 256 * 256;" in api
    assert "const int64_t cap = bin_capacity_from_bytes(per_view);" in api
    assert "size_t gsr_binning_bytes(int64_t R) { return bin_view(nullptr, R).bytes + 256; }" in api


# ---- the documentation ----------------------------------------------------------------------------------------------------------
def test_every_row_of_the_arena_contract_table_names_an_existing_case():
    text = open(os.path.join(util.ROOT, "DESIGN.md")).read()
    start = text.index("**The arena contract.**")
    rows = [ln for ln in text[start:text.index("\n## 7.", start)].splitlines() if ln.startswith("| ")][1:]     # (without the header)
    assert len(rows) >= 25, len(rows)
    named = set()
    for ln in rows:
        cells = [c.strip() for c in ln.strip().strip("|").split("|")]
        assert len(cells) == 6, ln
        cases = re.findall(r"`([a-z_]+)`", cells[5])
        assert cases and all(c in AC.CASES for c in cases), ln
        named.update(cases)
    assert named == set(AC.CASES), sorted(set(AC.CASES) - named)
    for view in ("GeomView", "ImageView", "BinView", "XStateView", "records"):
        assert any(view in ln.split("|")[1] for ln in rows), view
