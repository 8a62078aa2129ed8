"""tests/fp64_channels.py on its own: the float64 extra-channel reference against the plain-C oracle (no GPU).

An extra-channel render with values x and view scale s is a colors_precomp render with colours x * s, so the reference's images
must be the oracle's float32 images of that run, and its dL/d extra the oracle's float64 render backward's dL_dcolor times s."""
import numpy as np
import pytest

import util
from fp64_channels import extra_render_fp64

SCENES = ["one_gaussian", "opaque_early_stop", "culled_mix", "deep_stack"]


def _run(oracle, name, nx=3, seed=0):
    s = util.build_scene(name)
    rng = np.random.default_rng(seed)
    P = s.P
    x = rng.normal(0, 1, (P, nx)).astype(np.float32)
    scale = np.array([-2.0, 0.5, 3.0][:nx], np.float32)
    bgx = rng.uniform(0, 1, nx).astype(np.float32)
    dl = rng.uniform(-1, 1, (nx, s.H, s.W)).astype(np.float32)
    kw = dict(W=s.W, H=s.H, tanfovx=s.tanfovx, tanfovy=s.tanfovy, bg=bgx, means3D=s.means3D, opacities=s.opacities,
              viewmatrix=s.viewmatrix, projmatrix=s.projmatrix, campos=s.campos, scales=s.scales, rotations=s.rotations,
              colors_precomp=x * scale[None, :])
    sx = util.Scene(**kw)
    fwd, gr = oracle.forward_backward(sx, dl, exact=True, nthreads=8)
    return s, x, scale, bgx, dl, fwd, gr


@pytest.mark.parametrize("name", SCENES)
def test_extra_gradient_is_the_oracle_float64_colour_gradient(oracle, name):
    s, x, scale, bgx, dl, fwd, gr = _run(oracle, name)
    r = extra_render_fp64(fwd, x, bgx, dl, scale=scale)
    want = gr["exact"]["dL_dcolor"] * scale.astype(np.float64)[None, :]
    assert np.abs(want).max() > 0, name
    err = np.abs(r["grad"] - want).max() / np.abs(want).max()
    assert err <= 1e-9, (name, err)
    # entries the pixels never took have exactly zero gradient, like the oracle's
    assert np.array_equal(r["grad"] == 0, want == 0), name


@pytest.mark.parametrize("name", SCENES)
def test_extra_images_are_the_oracle_float32_images(oracle, name):
    s, x, scale, bgx, dl, fwd, gr = _run(oracle, name)
    r = extra_render_fp64(fwd, x, bgx, scale=scale)
    img32 = fwd["out_color"].astype(np.float64)
    # float32 compositing of up to 20 000 entries against the float64 sum: a few ulp of the largest partial sums
    mag = np.abs(x * scale).max() + np.abs(bgx).max()
    err = np.abs(r["image"] - img32).max()
    assert err <= 1e-5 * mag, (name, err, mag)
    assert r["grad"] is None
    # final_T: the replayed float64 transmittance against the oracle's float32 one
    assert np.abs(r["final_T"] - fwd["final_T"]).max() <= 1e-5, name


@pytest.mark.parametrize("name", SCENES)
def test_extra_gradient_is_the_central_difference_of_the_image(oracle, name):
    """The image is linear in the values: a float64 central difference of L = sum image * dL_dextra along a direction that moves a
    few values reproduces grad . direction to ~1e-10 (float64 values: the reference then composites x * scale unrounded)."""
    s, x, scale, bgx, dl, fwd, gr = _run(oracle, name)
    x64 = x.astype(np.float64)
    r = extra_render_fp64(fwd, x64, bgx, dl, scale=scale)
    dl64 = dl.astype(np.float64)
    touched = np.nonzero(np.abs(r["grad"]).sum(1) > 0)[0]
    assert touched.size > 0, name
    rng = np.random.default_rng(1)
    rows = rng.choice(touched, min(6, touched.size), replace=False)
    d = np.zeros_like(x64)
    d[rows] = rng.uniform(-1, 1, (rows.size, x.shape[1]))
    h = 0.25
    lp = (extra_render_fp64(fwd, x64 + h * d, bgx, scale=scale)["image"] * dl64).sum()
    lm = (extra_render_fp64(fwd, x64 - h * d, bgx, scale=scale)["image"] * dl64).sum()
    fd, want = (lp - lm) / (2 * h), (r["grad"] * d).sum()
    assert abs(fd - want) <= 1e-10 * max(np.abs(r["grad"][rows]).max(), 1e-3), (name, fd, want)
    # and a value no pixel takes moves nothing
    if touched.size < x.shape[0]:
        i = np.setdiff1d(np.arange(x.shape[0]), touched)[0]
        d2 = np.zeros_like(x64)
        d2[i] = 1.0
        a = extra_render_fp64(fwd, x64 + d2, bgx, scale=scale)["image"]
        b = extra_render_fp64(fwd, x64, bgx, scale=scale)["image"]
        assert np.array_equal(a, b), name
