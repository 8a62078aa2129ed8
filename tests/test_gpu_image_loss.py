"""The fused photometric loss on the device (gsr_image_loss_forward / gsr_image_loss_backward, pcrender.losses) against the float64
reference of image_loss_ref, on the smallest shapes at which the kernels can go wrong (the case table names them with the kernel's
own tile constants; the `long` cases have more partial sums than the sum kernel has lanes).  Every output is prefilled with NaN
before every call.

Accuracy bars (per view, none taken from the kernel's own results): the gradient metric e = max|g - g64| / max|g64| is at most
max(4 e32, 64 2^-24), e32 being the float32 torch formulation's e on the same case -- 4 for the other summation order (two 11-tap
passes against one 121-tap pass) on top of an error of the same origin, the floor half the worst-case rounding of a 121-term float32
sum; the first three loss terms are within max(4 e32_term, 8 2^-24) of float64, absolutely; the fourth equals
(1 - lambda) [0] + lambda (1 - [1]) of the returned float32 values (lambda as the float32 the C ABI takes) to one rounding.
image == target: the float64 gradient is analytically 0 and numerically rounding noise, so the ratio says nothing there; the
library's gradient has to be exactly 0 (the header's promise), which satisfies the ratio's bar for any noise."""
import numpy as np
import pytest
import torch

import image_loss_ref as R
import native_calls as NC
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    from diff_gaussian_rasterization import _native
    return _native


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _case(name):
    return next(c for c in R.CASES if c.name == name)


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_terms_and_gradient_against_float64(N, dev, c):
    before = N.lib.gsr_d2h_count()
    r = R.measure(N, c, dev)
    assert N.lib.gsr_d2h_count() == before
    print("%s: e %s e32 %s e/e32 %s term errors %s (float32 formulation %s)"
          % (c.name, r["e"], r["e32"], r["e"] / np.maximum(r["e32"], 1e-300), r["term_err"].tolist(), r["term_err32"].tolist()))
    assert np.isfinite(r["terms"]).all() and np.isfinite(r["grad"]).all()       # every element written
    if c.content == "identical":
        assert not r["grad"].any() and (r["terms"][:, 0] == 0).all() and (r["terms"][:, 2] == 0).all()
    for v in range(c.V):
        assert r["e"][v] <= max(4 * r["e32"][v], R.GRAD_FLOOR), (c.name, v, r["e"][v], r["e32"][v])
        for k in range(3):
            assert r["term_err"][v, k] <= max(4 * r["term_err32"][v, k], R.TERM_FLOOR), (c.name, v, k, r["term_err"][v], r["term_err32"][v])
        t = r["terms"][v]
        lam = float(np.float32(c.lam))
        want = (1.0 - lam) * t[0] + lam * (1.0 - t[1])
        assert abs(t[3] - want) <= 2.0 ** -24 * abs(want), (c.name, v, t, want)


def _assert_the_bars(c, r, what):
    """the module's bars on figures of image_loss_ref.figures: the terms, and the gradient where there is one"""
    assert np.isfinite(r["terms"]).all()
    for v in range(c.V):
        for k in range(3):
            assert r["term_err"][v, k] <= max(4 * r["term_err32"][v, k], R.TERM_FLOOR), (what, v, k, r["term_err"][v], r["term_err32"][v])
        if "e" in r:
            assert np.isfinite(r["grad"]).all() and r["e"][v] <= max(4 * r["e32"][v], R.GRAD_FLOOR), (what, v, r["e"][v], r["e32"][v])


@pytest.mark.parametrize("name", ["long", "long,odd"])
def test_metrics_only_forward_past_the_sum_kernel_s_lanes(N, dev, name):
    """more (tile, channel) pairs than IL_THREADS: the metrics-only walk adds pair i to accumulator i % IL_THREADS, the state path's
    k_image_loss_sum gives lane t the partials i = t mod IL_THREADS -- both against float64, and the same bits (the header's promise)"""
    c = _case(name)
    assert R.parts(c) > R.IL_THREADS
    with_state, _, _ = R.run_library(N, c, dev)
    metrics, _, _ = R.run_library(N, c, dev, with_state=False)
    r = R.figures(c, metrics)
    print("%s: term errors %s (float32 formulation %s)" % (c.name, r["term_err"].tolist(), r["term_err32"].tolist()))
    _assert_the_bars(c, r, c.name + " metrics only")
    _assert_the_bars(c, R.figures(c, with_state), c.name + " with a state")
    assert torch.equal(metrics, with_state)


@pytest.mark.parametrize("name", ["40x24", "long"])
def test_misaligned_pointers_with_16_byte_rows_carry_the_aligned_bits(N, dev, name):
    """W % 4 == 0 on pointers 4 B off a 16-B boundary: image and target (element loads and stores in both directions), then the
    gradient alone (a 16-B forward followed by an element backward).  The path does not enter a result."""
    c = _case(name)
    assert c.W % 4 == 0 and c.ss == 1
    terms, grad, _ = R.run_library(N, c, dev)
    _assert_the_bars(c, R.figures(c, terms, grad), c.name)
    for shift_inputs, shift_out in ((0, 0), (1, 0), (0, 1)):           # (the first: the 16-B path itself between the guard words)
        t, g = R.run_library_offset(N, c, dev, shift_inputs, shift_out)
        _assert_the_bars(c, R.figures(c, t, g), (c.name, shift_inputs, shift_out))
        assert torch.equal(t, terms) and torch.equal(g, grad), (c.name, shift_inputs, shift_out)


@pytest.mark.parametrize("name", ["64x48,V=3", "ss2,17x16,V=3"])
def test_bits_repeat_views_are_independent_and_upstream_gradients_scale(N, dev, name):
    c = _case(name)
    before = N.lib.gsr_d2h_count()
    t1, g1, s1 = R.run_library(N, c, dev)
    t2, g2, s2 = R.run_library(N, c, dev)
    assert torch.equal(t1, t2) and torch.equal(g1, g2) and torch.equal(s1, s2)          # two identical calls: identical bits
    t0, _, _ = R.run_library(N, c, dev, with_state=False)                              # metrics only: the same loss_terms bits
    assert torch.equal(t0, t1)
    img, tgt = (torch.from_numpy(a.copy()).to(dev) for a in R.references(c)[:2])
    for v in range(c.V):                                                                # view v alone: the batch's bits
        state = N.image_loss_state(1, c.W, c.H, dev).fill_(255)
        tv = N.image_loss_forward(img[v:v + 1].contiguous(), tgt[v:v + 1].contiguous(), c.lam, c.ss, state=state)
        gv = N.image_loss_backward(img[v:v + 1].contiguous(), tgt[v:v + 1].contiguous(), c.lam, c.ss, state,
                                   out=torch.full_like(img[v:v + 1], float("nan")))
        assert torch.equal(tv[0], t1[v]) and torch.equal(gv[0], g1[v]), v
    # an upstream gradient: 0 silences a view, powers of two scale the others exactly; a repeated backward on one forward repeats
    _, gw, sw = R.run_library(N, c, dev, dL=[0.5, 0.0, 2.0])
    assert not gw[1].any() and torch.equal(gw[0], 0.5 * g1[0]) and torch.equal(gw[2], 2.0 * g1[2]) and g1[0].abs().max() > 0
    again = N.image_loss_backward(img, tgt, c.lam, c.ss, sw, dL_dloss=torch.tensor([0.5, 0.0, 2.0], device=dev),
                                  out=torch.full_like(img, float("nan")))
    assert torch.equal(again, gw)
    torch.cuda.synchronize()
    assert N.lib.gsr_d2h_count() == before


def test_state_offsets_past_four_gigabytes(N, dev):
    """9 views of 4096 x 4096: the last view's maps lie more than 2^32 bytes into the state block (the entries refuse frames of 2^31
    elements, so the frames' own offsets stay below that; every plane offset is 64-bit in the kernels and this is where a 32-bit one
    would show).  The last view has to equal the same view submitted alone, bit for bit -- no reference of this size is computed."""
    V, W, H = 9, 4096, 4096
    assert 9 * (V - 1) * W * H * 4 > 2 ** 32 and 3 * V * W * H < 2 ** 31
    g = torch.Generator(device=dev).manual_seed(5)
    img, tgt = torch.rand((V, 3, H, W), device=dev, generator=g), torch.rand((V, 3, H, W), device=dev, generator=g)
    state = N.image_loss_state(V, W, H, dev).fill_(255)
    terms = N.image_loss_forward(img, tgt, 0.2, 1, state=state)
    grad = N.image_loss_backward(img, tgt, 0.2, 1, state, out=torch.full_like(img, float("nan")))
    last = grad[V - 1].clone()
    assert torch.isfinite(terms).all() and torch.isfinite(grad).all() and last.abs().max() > 0
    del grad, state
    one, one_t = img[V - 1:].contiguous(), tgt[V - 1:].contiguous()
    del img, tgt
    state1 = N.image_loss_state(1, W, H, dev).fill_(255)
    terms1 = N.image_loss_forward(one, one_t, 0.2, 1, state=state1)
    grad1 = N.image_loss_backward(one, one_t, 0.2, 1, state1, out=torch.full_like(one, float("nan")))
    assert torch.equal(terms1[0], terms[V - 1]) and torch.equal(grad1[0], last)
    del one, one_t, state1, grad1, last
    torch.cuda.empty_cache()


def test_photometric_loss_is_the_c_abi_with_the_upstream_gradient(N, dev):
    from pcrender import losses
    c = _case("ss2,17x16,V=3")
    img, tgt = (torch.from_numpy(a.copy()).to(dev) for a in R.references(c)[:2])
    w = torch.tensor([0.75, 1.5, 0.3], device=dev)
    x = img.clone().requires_grad_(True)
    loss = losses.photometric_loss(x, tgt, c.lam, c.ss)
    (loss * w).sum().backward()
    terms, _, state = R.run_library(N, c, dev)
    want = N.image_loss_backward(img, tgt, c.lam, c.ss, state, dL_dloss=w, out=torch.full_like(img, float("nan")))
    assert loss.shape == (c.V,) and torch.equal(loss.detach(), terms[:, 3]) and torch.equal(x.grad, want)
    m = losses.image_metrics(img, tgt, c.ss)
    assert torch.equal(m["l1"], terms[:, 0]) and torch.equal(m["ssim"], terms[:, 1]) and torch.equal(m["mse"], terms[:, 2])
    assert m["psnr"].shape == (c.V,) and torch.isfinite(m["psnr"]).all()
    assert torch.allclose(m["psnr"], -10 * torch.log10(terms[:, 2]))


def _torch_loss(frames, target, lam):
    """the float32 torch formulation on the device, per view"""
    return R.loss_terms(frames, target, lam)[:, 3]


def test_one_training_step_end_to_end(dev):
    """rasterize_views -> photometric_loss -> backward(): the cloud's gradients agree with the same step under the torch loss"""
    import diff_gaussian_rasterization as d
    from pcrender import losses
    s = util.build_scene("random_aniso")
    a = NC.scene_args([s], dev)
    sts = NC.scene_settings([s], dev)
    target = torch.from_numpy(np.random.default_rng(3).random((1, 3, s.H, s.W)).astype(np.float32)).to(dev)
    grads = []
    for loss_fn in (lambda f: losses.photometric_loss(f, target, 0.2), lambda f: _torch_loss(f, target, 0.2)):
        leaves = {k: a[i].clone().requires_grad_(True) for k, i in (("means3D", NC.MEANS3D), ("opacities", NC.OPACITIES),
                                                                    ("scales", NC.SCALES), ("rotations", NC.ROTATIONS))}
        colour = dict(shs=a[NC.SHS].clone().requires_grad_(True)) if a[NC.SHS].numel() else dict(
            colors_precomp=a[NC.COLORS].clone().requires_grad_(True))
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
        frames, _ = d.rasterize_views(leaves["means3D"], means2D, leaves["opacities"], sts, scales=leaves["scales"],
                                      rotations=leaves["rotations"], **colour)
        assert tuple(frames.shape) == (1, 3, s.H, s.W)      # exactly as returned: no finish, no copy
        loss_fn(frames).sum().backward()
        got = dict(leaves, **colour)
        grads.append({k: t.grad.detach().cpu().numpy().astype(np.float64) for k, t in got.items()})
    fused, ref = grads
    names = {"means3D": "dL_dmean3D", "opacities": "dL_dopacity", "scales": "dL_dscale", "rotations": "dL_drot", "shs": "dL_dsh",
             "colors_precomp": "dL_dcolor"}
    gp = {names[k]: v for k, v in fused.items()}
    go = {names[k]: v for k, v in ref.items()}
    assert max(np.abs(v).max() for v in go.values()) > 0
    util.check_grads(gp, go, "photometric step", names=tuple(gp))
