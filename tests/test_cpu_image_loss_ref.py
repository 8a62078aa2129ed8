"""The float64 reference of the photometric loss (image_loss_ref) held to three things that do not share its code: the formula
evaluated pixel by pixel, central differences of its own loss, and the bilinear down-filter its ss = 2 path stands for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_loss_ref as R


@pytest.mark.parametrize("W,H", [(5, 7), (12, 13)])
def test_reference_equals_the_formula_pixel_by_pixel(W, H):
    rng = np.random.default_rng(W * 100 + H)
    img, tgt = rng.random((2, 3, H, W)), rng.random((2, 3, H, W))
    terms, _ = R.loss_and_grad(img, tgt, 0.2)
    for v in range(2):
        want = R.brute_terms(img[v], tgt[v], 0.2)
        assert np.abs(terms[v] - want).max() < 1e-13, (v, terms[v], want)


@pytest.mark.parametrize("ss", [1, 2])
def test_reference_gradient_equals_central_differences(ss):
    W, H, lam = 9, 8, 0.3
    rng = np.random.default_rng(77 + ss)
    img, tgt = rng.random((2, 3, H * ss, W * ss)), rng.random((2, 3, H, W))
    dL = np.array([0.5, 2.0])
    _, grad = R.loss_and_grad(img, tgt, lam, ss, dL=dL)
    Hs, Ws = H * ss, W * ss
    h = 1e-6
    for v, ch, i, j in ((0, 0, 0, 0), (0, 1, 0, Ws - 1), (1, 2, Hs - 1, 0), (1, 0, Hs - 1, Ws - 1), (0, 2, Hs // 2, Ws // 2), (1, 1, 3, 5)):
        vals = []
        for s in (+h, -h):
            p = img.copy()
            p[v, ch, i, j] += s
            vals.append(float((R.loss_terms(torch.from_numpy(p), torch.from_numpy(tgt), lam, ss)[:, 3].numpy() * dL).sum()))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - grad[v, ch, i, j]) < 1e-8 + 1e-6 * abs(fd), (v, ch, i, j, fd, grad[v, ch, i, j])


def test_rate_two_is_the_bilinear_down_filter():
    a = torch.from_numpy(np.random.default_rng(5).random((2, 3, 14, 18)))
    assert torch.equal(F.interpolate(a, size=(7, 9), mode="bilinear", align_corners=False), F.avg_pool2d(a, 2))
    tgt = torch.from_numpy(np.random.default_rng(6).random((2, 3, 7, 9)))
    down = F.interpolate(a, size=(7, 9), mode="bilinear", align_corners=False)
    assert torch.equal(R.loss_terms(a, tgt, 0.2, ss=2), R.loss_terms(down, tgt, 0.2, ss=1))


def test_case_table_is_seeded_and_covers_the_kernel_paths():
    TW, TH = R.tile_constants()
    assert TW % 4 == 0 and TW >= 8 and TH >= 8
    sizes = {(c.W, c.H, c.ss) for c in R.CASES}
    for want in ((1, 1, 1), (5, 7, 1), (11, 11, 1), (TW, TH, 1), (TW + 1, TH + 1, 1), (40, 24, 1), (64, 48, 1), (8, 12, 2), (17, 16, 2)):
        assert want in sizes, want
    assert any(c.W % 2 == 1 and c.W % 4 != 0 for c in R.CASES) and {0.0, 0.2, 1.0} <= {c.lam for c in R.CASES}
    assert {"noise", "smooth", "constant", "identical"} == {c.content for c in R.CASES} and any(c.V == 3 for c in R.CASES)
    assert len({c.name for c in R.CASES}) == len(R.CASES) and len({c.seed for c in R.CASES}) == len(R.CASES)
    # more partial sums than k_image_loss_sum has lanes -- on 16-B rows, on element loads and at rate 2 -- and tile grids that are
    # wider than tall and taller than wide (il_tile's tile % tiles_x, tile / tiles_x), a single row and a single column of tiles
    long = [c for c in R.CASES if R.parts(c) > R.IL_THREADS]
    assert any(c.W % 4 == 0 and c.ss == 1 for c in long) and any(c.W % 4 != 0 and c.ss == 1 for c in long) and any(c.ss == 2 for c in long)
    assert R.parts(R.CASES[3]) == 3 and R.tiles(R.CASES[4]) == (2, 2)
    grids = {R.tiles(c) for c in R.CASES}
    assert any(x > y > 1 for x, y in grids) and any(y > x > 1 for x, y in grids) and {(3, 1), (1, 3)} <= grids
    assert any(c.ss == 2 and c.W % 4 != 0 and min(R.tiles(c)) > 1 for c in R.CASES)      # rate 2 on element loads across tile borders
    assert max(c.V * c.W * c.H * c.ss * c.ss for c in R.CASES) <= 2 ** 19                # the float64 reference stays a second or two
    for c in R.CASES[:3] + R.CASES[-2:]:
        a, b = R.case_inputs(c), R.case_inputs(c)
        assert a[0].shape == (c.V, 3, c.H * c.ss, c.W * c.ss) and a[1].shape == (c.V, 3, c.H, c.W) and a[0].dtype == np.float32
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = next(c for c in R.CASES if c.content == "identical")
    assert np.array_equal(*R.case_inputs(c))
    c = next(c for c in R.CASES if c.V == 3)
    img, _ = R.case_inputs(c)
    assert not np.array_equal(img[0], img[1]) and not np.array_equal(img[1], img[2])
