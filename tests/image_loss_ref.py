"""The photometric loss of include/gsr.h (gsr_image_loss_forward / gsr_image_loss_backward) in torch on the CPU, the seeded cases the
CPU and GPU tests share, and the comparison of the library against it.  Importable without the built library or a device.

  window / loss_terms / loss_and_grad     the definition: conv2d with the 121-tap window, avg_pool2d for ss = 2, autograd; float64 is
                                          the reference, float32 the yardstick for rounding (the formulation a trainer writes in torch)
  brute_terms                             the same formula pixel by pixel in numpy loops (what test_cpu_image_loss_ref holds it to)
  tile_constants / IL_THREADS             IL_TILE_W, IL_TILE_H, IL_THREADS as csrc/image_loss.hpp defines them
  CASES / case_inputs / tiles / parts     the case table: sizes, views, rate, lambda, content; inputs from the case's seed; a case's
                                          tile grid and the (tile, channel) partial sums of one of its views
  GRAD_FLOOR / TERM_FLOOR / grad_error    the accuracy bars' floors and the gradient metric e = max|g - g64| / max|g64| per view
  figures / measure                       the library's results of a case against both formulations: every figure the bars are about
  offset_view / guards_hold / run_library_offset   a tensor as a view some floats into a larger allocation of guard words; a case run
                                          on such views"""
import os
import re
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1, C2 = 1e-4, 9e-4
GRAD_FLOOR = 64 * 2.0 ** -24    # half the worst-case rounding of a 121-term float32 sum
TERM_FLOOR = 8 * 2.0 ** -24


def window(dtype):
    """[3,1,11,11]: the normalised separable Gaussian window, sigma 1.5, one copy per channel"""
    k = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(k - 5) ** 2 / 4.5)
    g = g / g.sum()
    return torch.outer(g, g).to(dtype).expand(3, 1, 11, 11).contiguous()


def loss_terms(image, target, lam, ss=1):
    """[V,4] loss terms of image [V,3,H ss,W ss] against target [V,3,H,W] in the tensors' dtype, differentiable"""
    x = F.avg_pool2d(image, 2) if ss == 2 else image
    y = target
    w = window(x.dtype).to(x.device)
    conv = lambda t: F.conv2d(t, w, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    m = (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    l1, ssim, mse = (x - y).abs().mean(dim=(1, 2, 3)), m.mean(dim=(1, 2, 3)), ((x - y) ** 2).mean(dim=(1, 2, 3))
    return torch.stack([l1, ssim, mse, (1 - lam) * l1 + lam * (1 - ssim)], dim=1)


def loss_and_grad(image, target, lam, ss=1, dtype=torch.float64, dL=None):
    """(terms [V,4], d sum_v dL[v] terms[v][3] / d image) as float64 numpy arrays, evaluated in `dtype` on the CPU"""
    x = torch.as_tensor(image).to(dtype).clone().requires_grad_(True)
    t = loss_terms(x, torch.as_tensor(target).to(dtype), lam, ss)
    wv = torch.ones(t.shape[0], dtype=dtype) if dL is None else torch.as_tensor(dL).to(dtype)
    (t[:, 3] * wv).sum().backward()
    return t.detach().double().numpy(), x.grad.double().numpy()


def brute_terms(image, target, lam):
    """the first three terms and the loss of ONE view [3,H,W] against its target (ss = 1), float64, pixel by pixel"""
    g = np.exp(-(np.arange(11) - 5.0) ** 2 / 4.5)
    g /= g.sum()
    x, y = np.asarray(image, np.float64), np.asarray(target, np.float64)
    _, H, W = x.shape
    tot = 0.0
    for c in range(3):
        for i in range(H):
            for j in range(W):
                acc = np.zeros(5)
                for di in range(-5, 6):
                    for dj in range(-5, 6):
                        a, b = i + di, j + dj
                        if 0 <= a < H and 0 <= b < W:
                            wgt, xv, yv = g[di + 5] * g[dj + 5], x[c, a, b], y[c, a, b]
                            acc += wgt * np.array([xv, yv, xv * xv, yv * yv, xv * yv])
                mu1, mu2 = acc[0], acc[1]
                s1, s2, s12 = acc[2] - mu1 * mu1, acc[3] - mu2 * mu2, acc[4] - mu1 * mu2
                tot += (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    l1, ssim, mse = np.abs(x - y).mean(), tot / x.size, ((x - y) ** 2).mean()
    return np.array([l1, ssim, mse, (1 - lam) * l1 + lam * (1 - ssim)])


def _constants(*names):
    text = open(os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc", "image_loss.hpp")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, text).group(1)) for n in names)


def tile_constants():
    return _constants("IL_TILE_W", "IL_TILE_H")


TW, TH = tile_constants()
IL_THREADS, = _constants("IL_THREADS")      # the lanes of k_image_loss_sum: partial i goes to lane i % IL_THREADS
Case = namedtuple("Case", "name V W H ss lam content seed")
CASES = (
    Case("1x1", 1, 1, 1, 1, 0.2, "noise", 1),
    Case("5x7", 1, 5, 7, 1, 0.2, "noise", 2),                      # every window hangs over every border
    Case("11x11", 1, 11, 11, 1, 0.2, "noise", 3),
    Case("tile", 1, TW, TH, 1, 0.2, "noise", 4),                   # one exact tile each way
    Case("tile+1", 1, TW + 1, TH + 1, 1, 0.2, "noise", 5),
    Case("40x24", 1, 40, 24, 1, 0.2, "noise", 6),                  # 16-B rows, a partial tile
    Case("64x48,V=3", 3, 64, 48, 1, 0.2, "noise", 7),
    Case("3tiles", 1, 3 * TW, 3 * TH, 1, 0.2, "noise", 8),         # a tile with neighbours on every side
    Case("37x19", 1, 37, 19, 1, 0.2, "noise", 9),                  # odd, not a multiple of 4: element loads and stores
    Case("ss2,8x12", 1, 8, 12, 2, 0.2, "noise", 10),
    Case("ss2,17x16,V=3", 3, 17, 16, 2, 0.2, "noise", 11),
    Case("ss2,tile+4", 1, TW + 4, TH + 1, 2, 0.2, "smooth", 12),   # 16-B rows at rate 2, more than one tile
    Case("lambda0", 1, 40, 24, 1, 0.0, "noise", 13),
    Case("lambda1", 1, 40, 24, 1, 1.0, "noise", 14),
    Case("smooth", 1, 64, 48, 1, 0.2, "smooth", 15),               # the variance cancellation at its worst
    Case("smooth,37x19", 1, 37, 19, 1, 1.0, "smooth", 16),
    Case("constant", 1, 40, 24, 1, 0.2, "constant", 17),
    Case("identical", 1, 37, 19, 1, 0.2, "identical", 18),
    # more partial sums than k_image_loss_sum has lanes (its index wraps), and tile grids that are not square
    Case("long", 1, 11 * TW, 8 * TH, 1, 0.2, "noise", 19),                     # 264 parts, 11 x 8 tiles, 16-B rows
    Case("long,odd", 2, 11 * TW - 3, 8 * TH - 1, 1, 0.2, "smooth", 20),        # the same on element loads, partial last tiles both ways
    Case("ss2,long", 1, 9 * TW + 4, 10 * TH, 2, 0.2, "noise", 21),             # 300 parts at rate 2, taller than wide
    Case("ss2,odd,tiles", 1, TW + 5, 2 * TH + 3, 2, 0.2, "noise", 22),         # rate 2 on element loads across tile borders, 2 x 3 tiles
    Case("3x1", 1, 3 * TW, TH, 1, 0.2, "noise", 23),                           # one row of tiles
    Case("1x3", 1, TW, 3 * TH, 1, 0.2, "noise", 24),                           # ... and one column
)


def tiles(c):
    """(tiles_x, tiles_y) of a case's loss-resolution frame"""
    return -(-c.W // TW), -(-c.H // TH)


def parts(c):
    """the (tile, channel) partial sums of one view: il_parts of csrc/image_loss.hpp"""
    return tiles(c)[0] * tiles(c)[1] * 3


def case_inputs(c):
    """(image [V,3,H ss,W ss], target [V,3,H,W]) float32 numpy, different content in every view"""
    rng = np.random.default_rng(1000 + c.seed)
    Hs, Ws = c.H * c.ss, c.W * c.ss
    yy, xx = np.meshgrid(np.arange(Hs) / c.ss, np.arange(Ws) / c.ss, indexing="ij")
    img, tgt = [], []
    for v in range(c.V):
        if c.content == "smooth":      # a smooth pattern plus 2 % noise
            chans = np.stack([0.5 + 0.4 * np.sin(0.11 * (k + 1) * xx + 0.07 * (v + 1) * yy + k) for k in range(3)])
            a = chans + 0.02 * rng.standard_normal((3, Hs, Ws))
            b = chans[:, ::c.ss, ::c.ss] + 0.02 * rng.standard_normal((3, c.H, c.W))
        elif c.content == "constant":  # a constant image against a near-constant one
            a = np.full((3, Hs, Ws), 0.5)
            b = 0.5 + 1e-3 * rng.standard_normal((3, c.H, c.W))
        else:
            a = rng.random((3, Hs, Ws))
            b = a.copy() if c.content == "identical" else rng.random((3, c.H, c.W))
        img.append(a)
        tgt.append(b)
    return np.stack(img).astype(np.float32), np.stack(tgt).astype(np.float32)


def grad_error(g, g64):
    """per view: max|g - g64| / max|g64| (a reference gradient of exactly 0 leaves max|g|: 0 or inf)"""
    V = g64.shape[0]
    num, den = np.abs(g - g64).reshape(V, -1).max(axis=1), np.abs(g64).reshape(V, -1).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))


_REFS = {}


def references(c):
    """(image, target, terms64, grad64, terms32, grad32) of a case: computed once, shared, never written to"""
    if c.name not in _REFS:
        img, tgt = case_inputs(c)
        t64, g64 = loss_and_grad(img, tgt, float(np.float32(c.lam)), c.ss, torch.float64)
        t32, g32 = loss_and_grad(img, tgt, float(np.float32(c.lam)), c.ss, torch.float32)
        for a in (img, tgt, t64, g64, t32, g32):
            a.setflags(write=False)
        _REFS[c.name] = (img, tgt, t64, g64, t32, g32)
    return _REFS[c.name]


def run_library(N, c, dev, dL=None, with_state=True):
    """the case through the C ABI's wrappers, every output prefilled with NaN: (terms [V,4], grad or None, state) on the device"""
    img, tgt = references(c)[:2]
    x, y = torch.from_numpy(img.copy()).to(dev), torch.from_numpy(tgt.copy()).to(dev)
    state = None
    if with_state:
        state = N.image_loss_state(c.V, c.W, c.H, dev)
        state.fill_(255)     # all bits set: a NaN as float32 and as float64
    terms = N.image_loss_forward(x, y, c.lam, c.ss, state=state)
    grad = None
    if with_state:
        out = torch.full_like(x, float("nan"))
        grad = N.image_loss_backward(x, y, c.lam, c.ss, state, dL_dloss=None if dL is None else torch.tensor(dL, dtype=torch.float32, device=dev),
                                     out=out)
    return terms, grad, state


_GUARD = 0x7FC0FEED      # a NaN pattern no kernel produces
_PAD = 8                 # guard words on either side (a multiple of 4: `shift` alone decides the alignment)


def offset_view(t, shift, fill=None):
    """(whole allocation, view shaped like t): a copy of the float32 device tensor t -- or, with fill, that value -- `shift` floats
    past a 16-B boundary, inside an allocation whose other words hold a guard pattern"""
    n = t.numel()
    whole = torch.full((2 * _PAD + shift + n,), _GUARD, dtype=torch.int32, device=t.device).view(torch.float32)
    view = whole[_PAD + shift:_PAD + shift + n].view(t.shape)
    view.copy_(t) if fill is None else view.fill_(fill)
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (shift % 4 == 0)
    return whole, view


def guards_hold(whole, view):
    w, n = whole.view(torch.int32), view.numel()
    at = (view.data_ptr() - whole.data_ptr()) // 4
    return bool((w[:at] == _GUARD).all()) and bool((w[at + n:] == _GUARD).all())


def run_library_offset(N, c, dev, shift_inputs, shift_out):
    """The case with image and target `shift_inputs` floats and the gradient `shift_out` floats past a 16-B boundary (the state block
    starts 4 B into its allocation; the entry aligns it, as it does for every caller).  The forward goes through the C ABI itself so
    that loss_terms too lies between guard words.  Asserts that the words around every output and the inputs hold: (terms, grad)."""
    img, tgt = references(c)[:2]
    x0, y0 = torch.from_numpy(img.copy()).to(dev), torch.from_numpy(tgt.copy()).to(dev)
    held = dict(image=offset_view(x0, shift_inputs), target=offset_view(y0, shift_inputs),
                terms=offset_view(torch.empty((c.V, 4), device=dev), 1, fill=float("nan")),
                grad=offset_view(x0, shift_out, fill=float("nan")))
    x, y, terms, out = (held[k][1] for k in ("image", "target", "terms", "grad"))
    nbytes, pad = int(N.lib.gsr_image_loss_state_bytes(c.V, c.W, c.H)), 64 + 4
    block = torch.full((pad + nbytes + pad,), 0x5A, dtype=torch.uint8, device=dev)
    state = block[pad:pad + nbytes].fill_(255)
    rc = N.lib.gsr_image_loss_forward(c.V, c.W, c.H, c.ss, float(c.lam), x.data_ptr(), y.data_ptr(), terms.data_ptr(), state.data_ptr(),
                                      state.numel(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, N.lib.gsr_last_error()
    grad = N.image_loss_backward(x, y, c.lam, c.ss, state, out=out)
    assert grad.data_ptr() == out.data_ptr()
    for name, (whole, view) in held.items():
        assert guards_hold(whole, view), "%s: a word next to %s was written" % (c.name, name)
    assert bool((block[:pad] == 0x5A).all()) and bool((block[pad + nbytes:] == 0x5A).all()), "%s: a byte next to the state was written" % c.name
    assert torch.equal(x, x0) and torch.equal(y, y0)
    return terms.clone(), grad.clone()


def figures(c, terms, grad=None):
    """every figure the accuracy bars are about, per view, of the library's terms (and gradient) of a case: e, e32 (gradient),
    term_err, term_err32 ([V,3], absolute), terms, grad"""
    _, _, t64, g64, t32, g32 = references(c)
    terms = terms.cpu().double().numpy()
    out = dict(term_err=np.abs(terms[:, :3] - t64[:, :3]), term_err32=np.abs(t32[:, :3] - t64[:, :3]), terms=terms)
    if grad is not None:
        grad = grad.cpu().double().numpy()
        out.update(e=grad_error(grad, g64), e32=grad_error(g32, g64), grad=grad)
    return out


def measure(N, c, dev):
    """figures of the case run through the library"""
    terms, grad, _ = run_library(N, c, dev)
    return figures(c, terms, grad)
