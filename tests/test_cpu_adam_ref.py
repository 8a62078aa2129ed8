"""The yardsticks of the Adam step, before any kernel runs: the float64 restatement of adam_ref is torch.optim.Adam, with a mask it is
torch's Adam on the visible rows alone, and the float32 restatement -- the arithmetic the kernel is specified to perform -- stays
within the single-step bars on every case of the table, so the bars are reachable."""
import numpy as np
import pytest
import torch

import adam_ref as R


def _torch_adam(p0, grads, lr):
    """torch.optim.Adam in float64 on the CPU over the list of gradients, with the float32 values of the hyper-parameters"""
    p = torch.tensor(np.asarray(p0, np.float64), requires_grad=True)
    opt = torch.optim.Adam([p], lr=float(R.F(lr)), betas=(float(R.F(R.BETA1)), float(R.F(R.BETA2))), eps=float(R.F(R.ADAM_EPS)))
    for g in grads:
        p.grad = torch.tensor(np.asarray(g, np.float64))
        opt.step()
    st = opt.state[p]
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("width,lr", [(3, 1.6e-4), (48, 2.5e-3), (1, 5e-2)])
def test_float64_restatement_is_torch_adam_over_20_dense_steps(width, lr):
    rng = np.random.default_rng(width)
    p0 = rng.standard_normal((65, width))
    grads = [rng.standard_normal((65, width)) * 10.0 ** rng.uniform(-3, 1) for _ in range(20)]
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        p, m, v = R.adam64(p, g, m, v, lr, t)
    pt, mt, vt = _torch_adam(p0, grads, lr)
    print("relative differences: p %.3g m %.3g v %.3g" % (_rel(p, pt), _rel(m, mt), _rel(v, vt)))
    assert np.abs(p - p0).max() > 10 * float(R.F(lr))         # the 20 steps moved the parameters
    assert _rel(p, pt) <= 1e-12 and _rel(m, mt) <= 1e-12 and _rel(v, vt) <= 1e-12


def test_with_a_mask_it_is_torch_adam_on_the_visible_rows_and_nothing_else_moves():
    rng = np.random.default_rng(11)
    P, width, lr = 65, 3, 2.5e-3
    vis = R.mask("random30", P)
    assert 0 < vis.sum() < P
    p0 = rng.standard_normal((P, width))
    grads = [rng.standard_normal((P, width)) for _ in range(20)]
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        p, m, v = R.adam64(p, g, m, v, lr, t, vis)
    on = vis != 0
    pt, mt, vt = _torch_adam(p0[on], [g[on] for g in grads], lr)
    assert _rel(p[on], pt) <= 1e-12 and _rel(m[on], mt) <= 1e-12 and _rel(v[on], vt) <= 1e-12
    assert (p[~on] == p0[~on]).all() and not m[~on].any() and not v[~on].any()


def test_the_case_table_reaches_the_kernel_s_edges():
    assert (R.VEC, R.WAVE, R.BLOCK) == (4, 64, 4 * R.THREADS)
    single = [c for c in R.CASES if len(c.widths) == 1]
    assert {c.widths[0] for c in single} == set(R.WIDTHS)
    for w in R.WIDTHS:
        Ps = {c.P for c in single if c.widths[0] == w}
        assert {1, 5, R.WAVE - 1, R.WAVE, R.WAVE + 1, 257, R.rows_of_a_block(w) - 1, R.rows_of_a_block(w) + 1} <= Ps, (w, Ps)
        assert (R.rows_of_a_block(w) - 1) * w < R.BLOCK < (R.rows_of_a_block(w) + 1) * w
    assert {(c.P * c.widths[0]) % R.VEC for c in single} == {0, 1, 2, 3}
    assert any(len(c.widths) == 8 and len(set(c.widths)) > 4 for c in R.CASES)
    off = [c for c in R.CASES if c.offset_rows]
    assert off and all((c.offset_rows * w * 4) % 16 != 0 for c in off for w in c.widths if w in (3, 45))
    for c in R.CASES:     # the inputs avoid subnormal intermediates: the smallest product of the step is c2 g^2
        for p, g, m, v in R.case_inputs(c):
            assert 1e-6 * 0.999 <= np.abs(g).min() and np.abs(g).max() <= 1e2 * 1.001 and v.min() > 0
            assert (1 - float(R.F(R.BETA2))) * float(np.abs(g).min()) ** 2 > 2.0 ** -126


def _split_of(c):
    """(units, workgroups per group, rounds per group, how often each round is taken per group) of a case's call"""
    units, blocks = R.work_split(c.P, c.widths)
    rounds = [R.div_up(c.P * w, R.BLOCK) for w in c.widths]
    taken = [R.rounds_taken(c.P * w, nb, R.on_vector_path(c, w)) for w, nb in zip(c.widths, blocks)]
    return units, blocks, rounds, taken


@pytest.mark.parametrize("c", R.CASES + R.CAP_CASES + (R.BENCH_SHAPE,), ids=[c.name for c in R.CASES + R.CAP_CASES + (R.BENCH_SHAPE,)])
def test_work_split_takes_every_round_of_every_group_exactly_once(c):
    """the entry's block_end table and the kernel's two grid-stride loops, restated at the granularity of one round"""
    units, blocks, rounds, taken = _split_of(c)
    assert units == sum(rounds)
    assert all(nb >= 1 for nb in blocks), (c.name, blocks)
    assert sum(blocks) <= R.MAX_BLOCKS + len(c.widths) - 1, (c.name, blocks)
    for k, (r, t) in enumerate(zip(rounds, taken)):
        assert len(t) == r and (t == 1).all(), (c.name, k, np.flatnonzero(t != 1)[:5])
    if units <= R.MAX_BLOCKS:
        assert blocks == rounds                      # below the cap every round has its own workgroup


def test_the_cap_cases_are_what_they_claim_to_be():
    assert R.BLOCK == R.VEC * R.THREADS and [c.name for c in R.CAP_CASES] == list(R.CAP_CLAIMS)
    for c in R.CASES:                                # the first table stops short of the cap, which is why the second exists
        assert R.work_split(c.P, c.widths)[0] <= R.MAX_BLOCKS
    for c in R.CAP_CASES:
        units, blocks, rounds, _ = _split_of(c)
        second, floored = R.CAP_CLAIMS[c.name]
        assert units > R.MAX_BLOCKS, (c.name, units)
        assert units <= R.MAX_BLOCKS + R.MAX_BLOCKS // 16, (c.name, units)          # ... and just above it: no larger than it has to be
        for k in second:                             # a workgroup with (at least) two rounds
            assert rounds[k] > blocks[k], (c.name, k, rounds[k], blocks[k])
        for k in range(len(c.widths)):
            share = rounds[k] * R.MAX_BLOCKS // units
            assert (share == 0) == (k in floored) and blocks[k] == max(share, 1), (c.name, k, share)
    w48, off1, floor, cloud = R.CAP_CASES
    assert R.work_split(w48.P, w48.widths) == (R.MAX_BLOCKS + 1, [R.MAX_BLOCKS]) and R.on_vector_path(w48, 48)
    assert 0 < (w48.P * 48) % R.BLOCK < R.BLOCK      # workgroup 0's second round is a partial one
    assert off1.offset_rows == 1 and not any(R.on_vector_path(off1, w) for w in off1.widths)
    assert floor.widths[1] == R.MAX_BLOCKS + 1 and floor.widths[1] % 2 == 1 and floor.P * floor.widths[0] <= R.BLOCK
    assert cloud.widths == R.BENCH_SHAPE.widths and (cloud.P * 3) % R.VEC != 0 and cloud.P % R.VEC != 0
    assert all(R.on_vector_path(cloud, w) for w in cloud.widths)
    # the two halves of the cloud case: together every row, each below the cap, the cut no multiple of 4
    (a0, b0), (a1, b1) = R.CAP_CLOUD_HALVES
    assert (a0, b0, b1) == (0, a1, cloud.P) and a1 % R.VEC != 0
    assert all(R.work_split(b - a, cloud.widths)[0] <= R.MAX_BLOCKS for a, b in R.CAP_CLOUD_HALVES)
    # the share arithmetic itself, on hand values: a round each up to the cap, floored shares above it, never none
    assert R.group_blocks(5 * R.BLOCK + 1, R.MAX_BLOCKS) == 6 and R.group_blocks(5 * R.BLOCK + 1, R.MAX_BLOCKS + 1) == 5
    assert R.group_blocks(1, 10 * R.MAX_BLOCKS) == 1 and R.group_blocks(30 * R.BLOCK, 10 * R.MAX_BLOCKS) == 3
    # the benchmark cloud runs the capped path with several rounds per workgroup
    units, blocks, rounds, _ = _split_of(R.BENCH_SHAPE)
    assert units > 2 * R.MAX_BLOCKS and all(r >= 2 * b for r, b in zip(rounds, blocks))
    # the mask kernel's own stride loop needs more Gaussians than its capped grid has lanes
    assert R.div_up(R.VISIBLE_CAP_P, R.THREADS) == R.MAX_BLOCKS + 1
    # the inputs of the big cases are the table's: no subnormal intermediate
    p, g, m, v = R.case_inputs(floor)[0]
    assert 1e-6 * 0.999 <= np.abs(g).min() and np.abs(g).max() <= 1e2 * 1.001 and v.min() > 0


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_float32_restatement_meets_the_single_step_bars(c):
    worst = np.zeros(3)
    for k, kind in enumerate((None,) + R.MASKS):
        vis = None if kind is None else R.mask(kind, c.P)
        for t in R.TS:
            for (lr, w, inp) in zip(c.lrs, c.widths, R.case_inputs(c, seed=k)):
                got = R.adam32(*inp, lr, t, vis)
                worst = np.maximum(worst, R.check_step(got, inp, lr, t, vis, what="%s %s t=%d w=%d" % (c.name, kind, t, w)))
    print("%s: worst error / bar  m %.3f  v %.3f  p %.3f" % (c.name, *worst))


def test_zero_gradient_and_moments_leave_the_parameter_alone():
    p = np.random.default_rng(1).standard_normal((5, 3)).astype(R.F)
    z = np.zeros_like(p)
    for fn in (R.adam32, R.adam64):
        p2, m2, v2 = fn(p, z, z, z, 1e-2, 1)
        assert (p2 == p).all() and not m2.any() and not v2.any()
