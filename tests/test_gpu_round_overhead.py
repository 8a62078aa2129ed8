"""The once-per-round code of the render kernels on the scenes of tests/round_cases.py: above all the footprint test, which bounds
a splat's reach over the live box from the edges that face its centre and takes the hardware reciprocal and logarithm
(csrc/tile_cull.hpp).  A test that drops an entry it must keep changes an image, n_contrib or a gradient here.
tests/test_cpu_round_cases.py shows on the CPU that these scenes produce splat centres inside, beside and diagonal to the live
boxes, live boxes of one pixel, one row and one column, survivor counts of every residue mod 4, rounds without a survivor and
rounds in which all 64 survive, and lists of two and three slices.

Per scene, as one view (half-quadrant forward, 512-entry slices) and as a batch of two (8 x 8 forward, 1 024-entry slices):
  * forward with the reference's full lists: lists, n_contrib, final_T and the image bit for bit what the reference build gives;
  * the default (footprint-clipped) forward: the same image and radii bit for bit;
  * atomic backward on both: against the reference build's gradients through the ladder of tests/grad_ladder.py (float64 arbiter);
  * deterministic backward twice: bit-identical, and inside util.check_grads of the atomic result.
The channels kernels (NX = 4 / 8) run the two scenes with long and sparse lists: out_extra bit for bit the reference build's
renders of the same values, gradients against float64 with the bars of tests/test_gpu_channels_fp64.py."""
import numpy as np
import pytest
import torch

import round_cases as RC
import util
from fp64_pins import channel_inputs as _inputs, compare_batch as _compare_batch, ref_decomposition as _ref_decomposition
from grad_ladder import (MAX_CASE_FRACTION, MAX_CASE_FRACTION_REF_TOO, MAX_ROW_FRACTION, MAX_ROW_FRACTION_REF_TOO, Float64,
                         assert_exits_stay_rare, hold_to_reference, new_tally)
from native_calls import reference_lists, scene_args as _args, to_device as _t
from sweep_support import (check_view_against_reference as _check_view_against_reference, records_backward as _backward,
                           same_bits as _same_bits)

pytestmark = pytest.mark.gpu

NAMES = util.GRAD_NAMES
TALLY = new_tally()
W, H = RC.W, RC.H


@pytest.mark.parametrize("V", [1, 2])
@pytest.mark.parametrize("name", RC.NAMES)
def test_colour_forward_and_backward(name, V, gpu_device):
    from diff_gaussian_rasterization import _native as N
    dev = gpu_device
    ref = util.reference_build("strict")
    scenes = RC.scenes(name, V)
    P = scenes[0].P
    tag = "round scene %s V=%d" % (name, V)
    dL = np.random.default_rng(5).uniform(-1, 1, (V, 3, H, W)).astype(np.float32)
    dL_t = _t(dL, dev)
    args = _args(scenes, dev)
    rf, gr = [], None
    for v, s in enumerate(scenes):
        r, g = ref.forward_backward(s, dL[v])
        rf.append(r)
        gr = {k: g[k].astype(np.float64) for k in NAMES} if gr is None else {k: gr[k] + g[k] for k in NAMES}
    f64 = Float64(scenes, dL, nthreads=16)
    n_pairs = max(1, max(r["R"] for r in rf))

    with reference_lists(True):
        full = N.rasterize_gaussians_batch(*args, need_backward=True)
        for v in range(V):
            _check_view_against_reference(N, "%s view %d" % (tag, v), rf[v], full, v, V, P, W, H, "sh")
        gp, _ = _backward(N, args, full, dL_t, False)
        hold_to_reference(tag + " full lists", 77, gp, gr, f64, TALLY, label="round overhead")
        d1, r1 = _backward(N, args, full, dL_t, True, pairs=n_pairs)
        d2, r2 = _backward(N, args, full, dL_t, True, pairs=n_pairs)
        assert _same_bits(d1, d2) and np.array_equal(r1.view(np.uint32), r2.view(np.uint32)), tag + ": deterministic, second run"
        util.check_grads(d1, gp, tag + ": deterministic vs atomic", names=NAMES)
        hold_to_reference(tag + " full lists, deterministic", 77, d1, gr, f64, TALLY, label="round overhead")

        N.set_reference_lists(False)
        run = N.rasterize_gaussians_batch(*args, need_backward=True)
        assert run[0] == full[0] and torch.equal(run[1], full[1]) and torch.equal(run[2], full[2]), tag + ": clipped vs full lists"
        gp, _ = _backward(N, args, run, dL_t, False)
        hold_to_reference(tag + " clipped lists", 77, gp, gr, f64, TALLY, label="round overhead")
        d1, r1 = _backward(N, args, run, dL_t, True, pairs=n_pairs)
        d2, r2 = _backward(N, args, run, dL_t, True, pairs=n_pairs)
        assert _same_bits(d1, d2) and np.array_equal(r1.view(np.uint32), r2.view(np.uint32)), tag + ": deterministic, clipped lists"
        util.check_grads(d1, gp, tag + ": deterministic vs atomic, clipped lists", names=NAMES)


@pytest.mark.parametrize("V", [1, 2])
@pytest.mark.parametrize("nx", [4, 8])
@pytest.mark.parametrize("name", ["long", "sparse"])
def test_channels_forward_and_backward(name, nx, V, oracle, gpu_device):
    from diff_gaussian_rasterization import _native as N
    from fp64_channels import _groups
    ref = util.reference_build("strict")
    scenes = RC.scenes(name, V)
    P = scenes[0].P
    tag = "round scene %s V=%d nx=%d" % (name, V, nx)
    layout = 2 if nx == 8 else 1
    x, dense, sc, bgx, dpix, dx = _inputs(P, V, nx, layout, seed=60 + nx + V, H=H, W=W)
    with reference_lists(True):
        run = _compare_batch(N, oracle, scenes, x, dense, sc, bgx, dpix, dx, layout, gpu_device, tag, 1e-5)
    images = np.zeros((V, nx, H, W), np.float32)
    _ref_decomposition(ref, scenes, dense, sc, bgx, dpix, dx, images=images)
    out_x = run[3].cpu().numpy()
    for v in range(V):
        for ks in _groups(nx):
            assert out_x[v, ks].tobytes() == images[v, ks].tobytes(), "%s: out_extra of view %d, channels %s: %d pixels differ" % (
                tag, v, ks, int((out_x[v, ks] != images[v, ks]).sum()))
    _compare_batch(N, oracle, scenes, x, dense, sc, bgx, dpix, dx, layout, gpu_device, tag + " clipped lists", 1e-5)


def test_round_overhead_escape_hatches_stay_rare():
    """Runs after the cases above (same process): how many comparisons / rows needed a fallback of the gradient ladder."""
    if TALLY["cases"] == 0:   # (selected alone)
        return
    print("round overhead tally:", TALLY)
    assert_exits_stay_rare(TALLY, MAX_CASE_FRACTION, MAX_ROW_FRACTION, MAX_CASE_FRACTION_REF_TOO, MAX_ROW_FRACTION_REF_TOO)
