"""The numpy restatement of adaptive density control (density_ref) against a literal torch transcription of 3DGS's three-stage
densify_and_prune (clone, then split, then prune; Kerbl et al., gaussian_model.py) on the shared cases, as a MULTISET of rows -- the
orders differ by design -- with the noise passed in; the census of the cases; the generator through two code paths and against the
published known-answer vectors of Philox4x32-10; the moments of the noise; and the float32 geometry against the float64 one.

The transcription differs from 3DGS's text where the library's interface does: the thresholds come from the rule (3DGS derives them
from the scene extent and ties the world-size test to the screen-size one), scales are stored linear or as logarithms, the averaged
gradient divides by max(views, 1) where 3DGS zeroes its NaN, and the normal draws are passed in instead of torch.normal.  The cases
keep max_world_size above dense_size, where the two definitions give the same rows (a clone never exceeds the world size)."""
import numpy as np
import pytest
import torch

import density_ref as R


def _transcription(inp):
    """3DGS's densify_and_prune on torch-CPU tensors, float64 geometry, decisions on the float32 values: (tag, rows per group), in
    3DGS's order (kept, then clones, then children) after its prune"""
    rule, P = inp["rule"], inp["P"]
    act = (lambda s: torch.exp(s)) if rule.log_scales else (lambda s: s)
    inv = (lambda s: torch.log(s)) if rule.log_scales else (lambda s: s)
    stored = torch.from_numpy(inp["scales"]).double()
    cloud = dict(xyz=torch.from_numpy(inp["means3D"]).double(), scaling=stored, rotation=torch.from_numpy(inp["rotations"]).double(),
                 opacity=torch.from_numpy(inp["opacities"]).reshape(-1, 1), tag=torch.arange(P).reshape(-1, 1),
                 shs=torch.from_numpy(inp["shs"]), mask=torch.zeros(P, dtype=torch.bool) if inp["prune_mask"] is None
                 else torch.from_numpy(inp["prune_mask"]).bool(), noise=torch.from_numpy(inp["noise"]).double())
    max_radii2D = torch.from_numpy(inp["max_radius"]).clone()
    # decisions compare the float32 values the kernel compares (linear scales), or float64 ones (log scales: rows near a threshold
    # are left out by the caller)
    scaling = lambda: act(cloud["scaling"]).float() if not rule.log_scales else act(cloud["scaling"])  # noqa: E731
    grads = torch.from_numpy(inp["grad_norm_sum"]) / torch.from_numpy(inp["visible_views"]).clamp(min=1).float()
    grads[grads.isnan()] = 0.0

    def postfix(new):
        for k in cloud:
            cloud[k] = torch.cat([cloud[k], new[k]], 0)

    # densify_and_clone
    selected = (grads >= float(rule.grad_threshold)) & (scaling().max(1).values <= float(rule.dense_size))
    postfix({k: v[selected] for k, v in cloud.items()})
    max_radii2D = torch.cat([max_radii2D, torch.zeros(int(selected.sum()), dtype=max_radii2D.dtype)])
    # densify_and_split
    n_init = cloud["xyz"].shape[0]
    padded = torch.zeros(n_init)
    padded[:P] = grads
    selected = (padded >= float(rule.grad_threshold)) & (scaling().max(1).values > float(rule.dense_size))
    stds = act(cloud["scaling"][selected]).repeat(2, 1)
    samples = torch.cat([cloud["noise"][selected][:, 0], cloud["noise"][selected][:, 1]], 0) * stds     # torch.normal(0, stds)
    q = cloud["rotation"][selected]
    if rule.normalize_rotations:
        q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rots = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3).repeat(2, 1, 1)
    new = {k: v[selected].repeat(*([2] + [1] * (v.dim() - 1))) for k, v in cloud.items()}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + cloud["xyz"][selected].repeat(2, 1)
    new["scaling"] = inv(act(cloud["scaling"][selected]).repeat(2, 1) / (0.8 * 2))
    postfix(new)
    max_radii2D = torch.cat([max_radii2D, torch.zeros(2 * int(selected.sum()), dtype=max_radii2D.dtype)])
    keep = ~torch.cat([selected, torch.zeros(2 * int(selected.sum()), dtype=torch.bool)])
    cloud = {k: v[keep] for k, v in cloud.items()}
    max_radii2D = max_radii2D[keep]
    # prune
    prune = (cloud["opacity"] < float(rule.min_opacity)).squeeze(1) | cloud["mask"]
    if rule.max_screen_radius > 0:
        prune |= max_radii2D > rule.max_screen_radius
    if rule.max_world_size > 0:
        prune |= scaling().max(1).values > float(rule.max_world_size)
    return {k: v[~prune].numpy() for k, v in cloud.items()}


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_restatement_gives_the_rows_of_3dgs_densify_and_prune(c):
    inp = R.case_inputs(c)
    rule, P = inp["rule"], inp["P"]
    assert float(rule.max_world_size) > float(rule.dense_size)
    action = R.case_actions(inp)
    tag = np.arange(P, dtype=np.float64).reshape(-1, 1)
    groups = [(inp["means3D"], R.MEANS), (inp["scales"], R.SCALES), (inp["shs"], R.COPY), (tag, R.COPY)]
    (xyz, scaling, shs, tags), index = R.apply_ref(rule, action, groups, inp["scales"], inp["rotations"], inp["noise"], np.float64)
    want = _transcription(inp)
    # rows of sources near a threshold (log scales only) may be decided either way: they leave both sides
    near = R.near_threshold(rule, inp["scales"]) if rule.log_scales else np.zeros(P, bool)
    assert near.sum() <= 1e-3 * P
    a_keep, b_keep = ~near[tags[:, 0].astype(int)], ~near[want["tag"][:, 0]]
    a = np.concatenate([tags, xyz, scaling.astype(np.float64), shs.astype(np.float64)], 1)[a_keep]
    b = np.concatenate([want["tag"].astype(np.float64), want["xyz"], want["scaling"], want["shs"].astype(np.float64)], 1)[b_keep]
    assert a.shape == b.shape, (c.name, a.shape, b.shape)
    a, b = a[np.lexsort((a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 1], b[:, 0]))]       # by source, then by x: a source's rows differ in x
    assert (a[:, 0] == b[:, 0]).all() and (a[:, 7:] == b[:, 7:]).all()
    assert np.allclose(a[:, 1:4], b[:, 1:4], rtol=1e-12, atol=1e-12)                     # float64 against float64
    assert np.allclose(a[:, 4:7], b[:, 4:7], rtol=3e-7, atol=0)                          # a float32 division or subtraction
    # the totals and the index say the same as the rows
    offsets, index2, totals = R.plan_of(action)
    assert (index == index2).all() and totals[0] == len(index) == offsets[-1]
    src = np.where(index >= 0, index, -1 - index)
    assert (np.diff(src) >= 0).all() and (np.bincount(src, minlength=P) == R.ROWS[action]).all()
    assert totals[1] == (index >= 0).sum() and totals[4] == (R.ROWS[action] == 0).sum()


def test_every_action_and_every_threshold_side_occurs_in_the_cases():
    inputs = [R.case_inputs(c) for c in R.CASES]
    codes, sides = R.census(inputs)
    assert (codes > 0).all(), codes
    assert all(s == {-1, 0, 1} for s in sides.values()), sides
    by_kind = {c.kind: R.case_actions(i) for c, i in zip(R.CASES, inputs)}
    assert (by_kind["all_pruned"] == R.PRUNED).all() and (by_kind["all_split"] == R.SPLIT).all() and (by_kind["all_kept"] == R.KEPT).all()
    assert {(c.log, c.norm) for c in R.CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {c.mask for c in R.CASES} == {0, 1}
    assert any(np.isnan(i["grad_norm_sum"]).any() and np.isinf(i["grad_norm_sum"]).any() and (i["visible_views"] == 0).any() for i in inputs)
    nan_rows = np.concatenate([R.case_actions(i)[np.isnan(i["grad_norm_sum"])] for i in inputs])
    assert len(nan_rows) and np.isin(nan_rows, (R.PRUNED, R.KEPT)).all()                 # a NaN gradient densifies nothing
    # the P that needs a second round of the scan of the workgroup counts, from the kernel's constants
    blocks = -(-R.TWO_ROUNDS_P // R.THREADS)
    assert blocks == R.SCAN_ROUND + 1 and any(c.P == R.TWO_ROUNDS_P for c in R.CASES)
    # ... and the P that needs a third
    assert -(-R.THREE_ROUNDS_P // R.THREADS) == 2 * R.SCAN_ROUND + 1 and R.CASES[-1].P == R.THREE_ROUNDS_P
    assert max(i["P"] for i in inputs) <= 300_000
    # the eight-group gather above its grid cap (DENSITY_MAX_BLOCKS rounds of DENSITY_BLOCK_ELEMS): some case's call has a workgroup
    # with a second round in EVERY group, and the last case's has workgroups with a third; every round is taken exactly once
    assert R.BLOCK == R.VEC * R.THREADS
    splits = {}
    for c, i in zip(R.CASES, inputs):
        groups = R.case_groups(i)
        widths = [int(np.prod(src.shape[1:])) for _, src, _ in groups]
        P_out = int(R.plan_of(R.case_actions(i))[2][0])
        units, blocks, rounds = splits[c.name] = R.apply_split(P_out, widths)
        assert sum(blocks) <= R.MAX_BLOCKS + len(widths) - 1 and all(b >= 1 for b in blocks) or P_out == 0
        for (_, _, role), w, nb, r in zip(groups, widths, blocks, rounds):
            vec = role in (R.COPY, R.MOMENT) and w % R.VEC == 0
            assert P_out == 0 or (R.adam_ref.rounds_taken(P_out * w, nb, vec, R.BLOCK) == 1).all(), (c.name, w)
    above = {name: s for name, s in splits.items() if s[0] > R.MAX_BLOCKS}
    print({name: s[0] for name, s in above.items()})
    assert any(all(r > b for b, r in zip(s[1], s[2])) for name, s in above.items() if name != R.CASES[-1].name), above
    units, blocks, rounds = splits[R.CASES[-1].name]
    assert units > 2 * R.MAX_BLOCKS and any(r > 2 * b for b, r in zip(blocks, rounds))
    # the log-scale cases leave fewer than 0.1 % of their rows out of the exact comparison
    for c, i in zip(R.CASES, inputs):
        if c.log:
            assert R.near_threshold(i["rule"], i["scales"]).sum() < 1e-3 * max(i["P"], 1000), c.name


def test_philox_two_code_paths_and_known_answers():
    # the known-answer vectors of Philox4x32-10 (Random123's kat_vectors)
    for counter, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                               ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                                (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert R.philox_scalar(counter, key) == want
        assert tuple(int(v) for v in R.philox(counter, key)) == want
    seed = 0xFEDCBA9876543210
    assert R.seed_key(seed) == (0x76543210, 0xFEDCBA98)
    i, k = np.meshgrid(np.array([0, 1, 2, 255, 70000, 2 ** 30 - 1]), np.arange(2), indexing="ij")
    words = R.philox((i, k, 0, 0), R.seed_key(seed))
    for a in range(i.shape[0]):
        for b in range(2):
            assert tuple(int(v) for v in words[a, b]) == R.philox_scalar((i[a, b], b, 0, 0), R.seed_key(seed))
    u = R.uniforms(np.array([0, 255, 256, 2 ** 31, 2 ** 32 - 1], np.uint32))
    assert u.dtype == np.float32 and (u > 0).all() and (u <= 1).all()
    assert u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24) and u[4] == 1.0


def test_noise_moments_over_2_to_the_20_draws():
    """mean and covariance of eps within 5 standard errors of 0 and I: for N independent standard normals the standard error of a
    mean is 1 / sqrt(N), of a sample variance sqrt(2 / N), of a sample covariance of two independent components 1 / sqrt(N)"""
    n = 1 << 20
    eps, _ = R.noise64(12345, n // 2)
    e = eps.reshape(-1, 3)
    assert e.shape == (n, 3) and np.isfinite(e).all()
    assert (np.abs(e.mean(0)) <= 5 / np.sqrt(n)).all(), e.mean(0)
    cov = e.T @ e / n
    bar = 5 * np.where(np.eye(3) > 0, np.sqrt(2.0 / n), np.sqrt(1.0 / n))
    assert (np.abs(cov - np.eye(3)) <= bar).all(), cov
    other, _ = R.noise64(12346, 1000)
    assert not np.array_equal(other, eps[:1000])                          # the seed enters
    assert np.array_equal(R.noise64(12345, 1000)[0], eps[:1000])          # ... and P does not


@pytest.mark.parametrize("name", ["mixed,P=1025", "mixed,P=1024", "mixed,P=257", "mixed,P=1023"])
def test_float32_geometry_against_float64_within_the_counted_roundings(name):
    inp = R.case_inputs(R.case(name))
    rule = inp["rule"]
    m32 = R.child_means(rule, inp["means3D"], inp["scales"], inp["rotations"], inp["noise"])
    m64 = R.child_means(rule, inp["means3D"], inp["scales"], inp["rotations"], inp["noise"], np.float64)
    bar = R.child_mean_bar(rule, m64, inp["scales"], inp["rotations"], inp["noise"])
    ratio = np.abs(m32.astype(np.float64) - m64) / bar
    print("%s: worst error / bar %.3f" % (name, ratio.max()))
    assert m32.dtype == np.float32 and (ratio <= 1).all()
    s32 = R.child_scales(rule, inp["scales"])
    s64 = R.sigma(rule, inp["scales"], np.float64) / 1.6
    assert (np.abs(R.sigma(rule, s32, np.float64) - s64) <= 4 * R.U * s64).all()
