"""The scenes of tests/round_cases.py do what tests/test_gpu_round_overhead.py needs them for: with the oracle's forward (the
lists the library walks when it runs with the reference's full lists) the CPU model of the backward's rounds
(round_cases.backward_rounds) must find every survivor residue mod 4 (padded last groups of every size), rounds without a
survivor and rounds in which all 64 survive, slices that end at a boundary inside a list, and the live boxes and centre
positions the footprint test is meant to meet."""
import numpy as np
import pytest

import round_cases as RC


@pytest.fixture(scope="module")
def stats(oracle):
    out = {}
    for name in RC.NAMES:
        for V in (1, 2):
            s = RC.scenes(name, V)[V - 1]
            assert s.W == 64 and s.H == 48 and s.P <= 3000
            f = oracle.forward(s)
            out[name, V] = (f, RC.backward_rounds(f, V))
    return out


@pytest.mark.parametrize("V", [1, 2])
@pytest.mark.parametrize("name", RC.NAMES)
def test_every_residue_and_every_centre_position(stats, name, V):
    f, st = stats[name, V]
    print(name, V, st, "padded places: %.1f %%" % (100.0 * (4 * st["groups"] - st["staged"]) / (4 * st["groups"])))
    assert min(st["residue"]) >= 10, st["residue"]          # survivor counts of every residue mod 4
    assert min(st["region"]) >= 100, st["region"]           # centres inside, beside and diagonal to the live box


@pytest.mark.parametrize("V", [1, 2])
def test_long_lists_cross_slice_boundaries(stats, V):
    f, st = stats["long", V]
    longest = int((f["ranges"][:, 1] - f["ranges"][:, 0]).max())
    assert longest > 1024 and st["slices_max"] == (3 if V == 1 else 2)
    assert st["last_inner_slice"] >= 3                      # slices that hand over to a checkpoint of the forward
    assert st["empty"] >= 10                                # rounds without a survivor between rounds with some
    assert f["final_T"].min() > 1e-3                        # no pixel terminates: every entry of the list is consumed


@pytest.mark.parametrize("V", [1, 2])
def test_sparse_scene_boxes_and_full_rounds(stats, V):
    f, st = stats["sparse", V]
    assert st["box_pixel"] >= 1 and st["box_row"] >= 1 and st["box_column"] >= 1
    assert st["full"] >= 1 and st["empty"] >= 1


@pytest.mark.parametrize("V", [1, 2])
def test_front_scene_terminates_pixels_at_different_depths(stats, V):
    f, st = stats["front", V]
    stopped = f["final_T"] < 1e-3
    assert 0.2 < stopped.mean() < 1.0
    # inside single quadrants: some pixels stopped early, others walked on (the forward's live box shrinks while it walks)
    n = f["n_contrib"].reshape(6, 8, 8, 8).transpose(0, 2, 1, 3).reshape(48, 64)
    assert (n.max(1) - n.min(1) > 64).sum() >= 10
