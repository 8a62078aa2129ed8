"""The two scratch-size queries of the deterministic backwards (gsr_backward_det_bytes, gsr_backward_det_channels_bytes) return
what they returned when tests/golden/det_scratch_sizes.json was recorded: callers allocate by these numbers and the library carves
by them, so a change of the plan's carving order or alignment shows here without a GPU.

    python tests/test_cpu_det_scratch_sizes.py --record     rewrites the fixture from the library in the tree
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "det_scratch_sizes.json")

GRID = {
    "V": [1, 2, 3, 12],
    "P": [0, 1, 997, 800000],
    "WH": [[16, 16], [96, 80], [1920, 1080]],
    "pairs": [0, 1, 4095, 4096, 4097, 1100000, 2 ** 32 - 1, 2 ** 32],
    # (nx, extra_per_view); nx = 0: the colour query
    "query": [[0, 0], [4, 0], [4, 1], [8, 0], [8, 1], [8, 2]],
}


def _sizes(grid):
    """the queries' answers over the grid, in itertools.product order of V, P, WH, pairs, query"""
    from diff_gaussian_rasterization import _native
    out = []
    for V, P, (W, H), pairs, (nx, layout) in itertools.product(*(grid[k] for k in ("V", "P", "WH", "pairs", "query"))):
        if nx == 0:
            out.append(int(_native.lib.gsr_backward_det_bytes(V, P, W, H, pairs)))
        else:
            out.append(int(_native.lib.gsr_backward_det_channels_bytes(V, P, W, H, pairs, nx, layout)))
    return out


def test_sizes_are_the_recorded_ones():
    with open(GOLDEN) as f:
        rec = json.load(f)
    assert rec["grid"] == GRID, "the fixture was recorded over another grid"
    got = _sizes(GRID)
    assert len(got) == len(rec["bytes"]) == 4 * 4 * 3 * 8 * 6
    assert min(got) > 0                                               # every point of the grid is a valid query
    keys = list(itertools.product(*(GRID[k] for k in ("V", "P", "WH", "pairs", "query"))))
    bad = [(k, g, w) for k, g, w in zip(keys, got, rec["bytes"]) if g != w]
    assert not bad, "%d of %d sizes differ from the recorded ones, first (V, P, WH, pairs, query), got, recorded: %r" % (
        len(bad), len(got), bad[0])


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, os.path.join(ROOT, "gaussian-pcloud-render_amd"))
    with open(GOLDEN, "w") as f:
        json.dump({"grid": GRID, "bytes": _sizes(GRID)}, f)
        f.write("\n")
    print("recorded %s" % GOLDEN)
