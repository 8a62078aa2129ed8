"""Adaptive density control on the device (gsr_density_plan / gsr_density_apply, pcrender.density) against the numpy restatement
(density_ref) on the shared cases: the smallest shapes at which the kernels can go wrong, named with the kernels' own constants.

  plan     offsets, action and totals equal the restatement exactly (float32 arithmetic of the same single operations).  log_scales cases
           decide on expf: the Gaussians whose float64 smax lies within 4 float32 ulp of a threshold are left out of the comparison of
           the action codes (fewer than 0.1 % of a case's rows, asserted), and offsets and totals are held to the device's own codes.
  apply    with caller noise and linear scales every output row of every group, and index, are bit-identical to the float32
           restatement, on the 16-B path and on the scalar path (every pointer 4 B off a 16-B boundary), which agree with each other, and
           without an index (rows found by bisection).  Every destination lies between guard words.  log_scales cases: every group but the
           means bit-identical, the children's means within density_ref.child_mean_bar of the float64 restatement.
  noise = NULL   the children's means against the float64 restatement from the same Philox integers, R and sigma being the float32
           values the definition prescribes: |mu' - (mu + d64)| <= sum_c |R_rc| sigma_c (16 U r_c + 3 U |eps_c|) + U |mu'|, U = 2^-24, r_c
           the Box-Muller radius of component c.  The 16 is counted: the rounding of the argument 2 pi u (at most 6.3 U), two library
           calls at 2 ulp = 4 U each, and the sqrt, product and constant roundings; 3 U for sigma * eps, R * t and the sums.  The bar
           rests on the math library's documented 2-ulp bounds for logf, sinf and cosf; the worst ratio is printed before it is asserted.
  properties, and one training loop through pcrender.density.densify_and_prune."""
import numpy as np
import pytest
import torch

import density_ref as R
import native_calls as NC

pytestmark = pytest.mark.gpu
GUARD = 0x7FC0DEAD                                                            # a NaN pattern no kernel produces
PAD = 8                                                                       # guard floats on either side (keeps 16-B alignment)


@pytest.fixture(scope="module")
def N():
    from diff_gaussian_rasterization import _native
    return _native


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _struct(N, rule):
    return N.DensityRuleStruct(float(rule.grad_threshold), float(rule.dense_size), float(rule.min_opacity), rule.max_screen_radius,
                               float(rule.max_world_size), rule.log_scales, rule.normalize_rotations, rule.seed)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(a, dev, shift, rows=None):
    """(whole buffer, view of `rows` rows like a's): a copy of `a` (or, with rows, an area of guard words) between PAD guard floats,
    `shift` floats off the 16-B boundary"""
    width = int(np.prod(a.shape[1:]))
    n = (a.shape[0] if rows is None else rows) * width
    big = torch.full((2 * PAD + n + shift,), GUARD, dtype=torch.int32, device=dev).view(torch.float32)
    view = big[PAD + shift:PAD + shift + n].view((-1,) + tuple(a.shape[1:])) if n else big[PAD + shift:PAD + shift].view((0,) + tuple(a.shape[1:]))
    if rows is None:
        view.copy_(NC.to_device(a, dev))
    assert n == 0 or (view.data_ptr() % 16 == 0) == (shift == 0)
    return big, view


def _guards_hold(big, n, shift):
    w = big.view(torch.int32)
    return bool((w[:PAD + shift] == GUARD).all()) and bool((w[PAD + shift + n:] == GUARD).all())


_PLANS = {}


def _plan(N, dev, c):
    """the case's inputs, the device's plan (tensors and numpy copies) and the restatement's action codes; made once per case"""
    if c.name not in _PLANS:
        inp = R.case_inputs(c)
        t = {k: None if inp[k] is None else NC.to_device(inp[k], dev)
             for k in ("scales", "opacities", "grad_norm_sum", "visible_views", "max_radius", "prune_mask", "rotations", "noise")}
        rule = _struct(N, inp["rule"])
        before = N.lib.gsr_d2h_count()
        offsets, action, totals = N.density_plan(rule, t["scales"], t["opacities"], t["grad_norm_sum"], t["visible_views"], t["max_radius"],
                                                 t["prune_mask"])
        assert N.lib.gsr_d2h_count() == before
        _PLANS[c.name] = dict(inp=inp, t=t, rule=rule, offsets=offsets, action=action, totals=totals,
                              h_offsets=offsets.cpu().numpy().view(np.uint32), h_action=action.cpu().numpy(),
                              h_totals=totals.cpu().numpy(), want=R.case_actions(inp))
    return _PLANS[c.name]


def _apply(N, dev, p, groups, shift=0, noise="caller", with_index=True, P_out=None):
    """gsr_density_apply of `groups` [(name, src array, role)] on guarded buffers; returns ({name: numpy rows}, index or None)"""
    n = int(p["h_totals"][0]) if P_out is None else P_out
    table, held = [], []
    for name, src, role in groups:
        _, s = _guarded(src, dev, shift)
        big, d = _guarded(src, dev, shift, rows=n)
        table.append((s, d, role))
        held.append((name, big, d))
    index = torch.full((n + 2,), GUARD, dtype=torch.int32, device=dev) if with_index else None
    if n == 0:      # an empty tensor has no address: the C ABI itself, with the addresses the rows would have had -- GSR_OK, nothing written
        import ctypes
        raw = (N.DensityGroup * len(table))(*[N.DensityGroup(s.data_ptr(), big.data_ptr() + 4 * (PAD + shift), s[0].numel(), role)
                                              for (s, _, role), (_, big, _) in zip(table, held)])
        assert N.lib.gsr_density_apply(s.shape[0], len(table), raw, ctypes.addressof(p["rule"]), p["offsets"].data_ptr(),
                                       p["action"].data_ptr(), p["t"]["scales"].data_ptr(), p["t"]["rotations"].data_ptr(), None,
                                       None if index is None else index[1:].data_ptr(), 0, None) == 0
    N.density_apply(table, p["rule"], p["offsets"], p["action"], n, scales=p["t"]["scales"], rotations=p["t"]["rotations"],
                    noise=p["t"]["noise"] if noise == "caller" else None, index=None if index is None else index[1:n + 1])
    out = {}
    for name, big, d in held:
        assert _guards_hold(big, d.numel(), shift), name
        out[name] = d.cpu().numpy()
    if index is not None:
        assert index[0] == GUARD and index[n + 1] == GUARD
        index = index[1:n + 1].cpu().numpy()
    return out, index


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_plan_equals_the_restatement(N, dev, c):
    p = _plan(N, dev, c)
    inp, want = p["inp"], p["want"]
    if c.log:
        near = R.near_threshold(inp["rule"], inp["scales"])
        assert near.sum() <= 1e-3 * inp["P"]
        print("%s: %d rows within 4 ulp of a threshold, %d of them decided otherwise" % (c.name, near.sum(), (p["h_action"] != want).sum()))
        assert (p["h_action"][~near] == want[~near]).all() and (p["h_action"] <= R.SPLIT).all()
        want = p["h_action"]
    else:
        assert (p["h_action"] == want).all(), np.flatnonzero(p["h_action"] != want)[:10]
    offsets, _, totals = R.plan_of(want)
    assert (p["h_offsets"] == offsets).all() and (p["h_totals"] == totals).all(), (p["h_totals"], totals)
    if c.kind == "all_pruned":
        assert totals[0] == 0 and totals[4] == inp["P"]
    if c.kind == "all_split":
        assert totals[0] == totals[3] == 2 * inp["P"]
    if c.kind == "all_kept":
        assert totals[0] == totals[1] == inp["P"]


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_apply_with_caller_noise_is_the_restatement_bit_for_bit(N, dev, c):
    p = _plan(N, dev, c)
    inp, rule = p["inp"], p["inp"]["rule"]
    groups = R.case_groups(inp)
    ref = [(src, role) for _, src, role in groups]
    want, want_index = R.apply_ref(rule, p["h_action"], ref, inp["scales"], inp["rotations"], inp["noise"])
    before = N.lib.gsr_d2h_count()
    aligned, index = _apply(N, dev, p, groups, shift=0)
    scalar, index1 = _apply(N, dev, p, groups, shift=1)
    bisect, none = _apply(N, dev, p, groups, shift=0, with_index=False)
    assert N.lib.gsr_d2h_count() == before and none is None
    assert (index == want_index).all() and (index1 == want_index).all()
    for (name, src, role), w in zip(groups, want):
        assert aligned[name].shape == w.shape == (len(want_index),) + src.shape[1:]
        assert (_bits(aligned[name]) == _bits(scalar[name])).all() and (_bits(aligned[name]) == _bits(bisect[name])).all(), name
        if role == R.MEANS and c.log:
            m64 = R.apply_ref(rule, p["h_action"], [(src, role)], inp["scales"], inp["rotations"], inp["noise"], np.float64)[0][0]
            src_row = np.where(want_index >= 0, want_index, -1 - want_index)
            split = p["h_action"][src_row] == R.SPLIT
            k = np.arange(len(src_row)) - p["h_offsets"][src_row].astype(np.int64)
            full64 = R.child_means(rule, src, inp["scales"], inp["rotations"], inp["noise"], np.float64)
            bar = R.child_mean_bar(rule, full64, inp["scales"], inp["rotations"], inp["noise"])[src_row[split], k[split]]
            ratio = np.abs(aligned[name][split].astype(np.float64) - m64[split]) / bar
            print("%s: children's means, worst error / bar %.3f" % (c.name, ratio.max() if ratio.size else 0.0))
            assert (ratio <= 1).all() and (_bits(aligned[name][~split]) == _bits(w[~split])).all()
        else:
            assert (_bits(aligned[name]) == _bits(w)).all(), (c.name, name, np.argwhere(_bits(aligned[name]) != _bits(w))[:5])
    if c.kind == "all_kept":                                              # the output equals the input bit for bit
        assert all((_bits(aligned[name]) == _bits(src)).all() for name, src, role in groups if role != R.MOMENT)
        assert (index == np.arange(inp["P"])).all()
    if c.kind == "all_pruned":
        assert len(index) == 0 and all(v.size == 0 for v in aligned.values())


GENERATED = ("mixed,P=257", "mixed,P=1024", "all_split,P=1025", "mixed,P=70001")


@pytest.mark.parametrize("name", GENERATED)
def test_apply_with_the_generator_against_float64_from_the_same_integers(N, dev, name):
    c = R.case(name)
    assert not c.log
    p = _plan(N, dev, c)
    inp, rule = p["inp"], p["inp"]["rule"]
    P = inp["P"]
    out, index = _apply(N, dev, p, [("means3D", inp["means3D"], R.MEANS)], noise=None)
    again, _ = _apply(N, dev, p, [("means3D", inp["means3D"], R.MEANS)], noise=None, shift=1)
    assert (_bits(out["means3D"]) == _bits(again["means3D"])).all()
    src = np.where(index >= 0, index, -1 - index)
    split = p["h_action"][src] == R.SPLIT
    k = (np.arange(len(src)) - p["h_offsets"][src].astype(np.int64))[split]
    i = src[split]
    assert split.sum() >= 2 and (_bits(out["means3D"][~split]) == _bits(inp["means3D"][src[~split]])).all()
    eps, radius = R.noise64(rule.seed, P)
    R32 = R.rotation(rule, inp["rotations"]).astype(np.float64)
    sig = R.sigma(rule, inp["scales"]).astype(np.float64)
    d64 = R.displacement(R32, sig, eps)[i, k]
    mu = inp["means3D"].astype(np.float64)[i]
    got = out["means3D"][split].astype(np.float64)
    term = np.abs(R32[i]) * (sig[i][:, None, :] * (16 * R.U * radius[i, k] + 3 * R.U * np.abs(eps[i, k]))[:, None, :])
    bar = term.sum(-1) + R.U * np.abs(got)
    ratio = np.abs(got - (mu + d64)) / bar
    print("%s: %d children, worst |mu' - (mu + d64)| / bar = %.4f" % (name, len(i), ratio.max()))
    assert (ratio <= 1).all(), ratio.max()


def test_bits_repeat_groups_and_row_ranges_are_independent(N, dev):
    c = R.case("mixed,P=1024")
    p = _plan(N, dev, c)
    inp = p["inp"]
    groups = R.case_groups(inp)
    whole, index = _apply(N, dev, p, groups)
    again, _ = _apply(N, dev, p, groups)
    assert all((_bits(whole[k]) == _bits(again[k])).all() for k in whole)                           # two identical calls
    t = p["t"]
    o2, a2, t2 = N.density_plan(p["rule"], t["scales"], t["opacities"], t["grad_norm_sum"], t["visible_views"], t["max_radius"], t["prune_mask"])
    assert torch.equal(o2, p["offsets"]) and torch.equal(a2, p["action"]) and torch.equal(t2, p["totals"])
    for j, g in enumerate(groups):                                                                  # every group alone, then in pairs
        alone, _ = _apply(N, dev, p, [g])
        pair, _ = _apply(N, dev, p, [groups[(j + 3) % len(groups)], g])
        assert (_bits(alone[g[0]]) == _bits(whole[g[0]])).all() and (_bits(pair[g[0]]) == _bits(whole[g[0]])).all(), g[0]
    # rows [a, b) planned and applied alone, with the rule's seed and the noise of the global rows: the bits of the whole call's rows
    for a, b in ((5, 1019), (255, 258), (1, 2)):
        cut = lambda x: None if x is None else x[a:b].contiguous()  # noqa: E731
        sub = dict(rule=p["rule"], t={k: cut(v) for k, v in t.items()})
        sub["offsets"], sub["action"], sub["totals"] = N.density_plan(p["rule"], sub["t"]["scales"], sub["t"]["opacities"],
                                                                      sub["t"]["grad_norm_sum"], sub["t"]["visible_views"],
                                                                      sub["t"]["max_radius"], sub["t"]["prune_mask"])
        sub["h_totals"] = sub["totals"].cpu().numpy()
        assert (sub["action"].cpu().numpy() == p["h_action"][a:b]).all()
        lo, hi = int(p["h_offsets"][a]), int(p["h_offsets"][b])
        assert sub["h_totals"][0] == hi - lo
        part, part_index = _apply(N, dev, sub, [(name, src[a:b], role) for name, src, role in groups])
        for name in whole:
            assert (_bits(part[name]) == _bits(whole[name][lo:hi])).all(), (name, a, b)
        assert (np.where(part_index >= 0, part_index + a, part_index - a) == index[lo:hi]).all()


def test_a_stale_P_out_truncates_and_never_writes_past_it(N, dev):
    c = R.case("mixed,P=1025")
    p = _plan(N, dev, c)
    groups = R.case_groups(p["inp"])
    whole, index = _apply(N, dev, p, groups)
    n = len(index)
    for short in (n - 1, n // 2, 1):                   # _apply's destinations hold `short` rows between their guards, which it checks
        for with_index in (True, False):
            part, part_index = _apply(N, dev, p, groups, P_out=short, with_index=with_index, shift=short % 2)
            assert all((_bits(part[k]) == _bits(whole[k][:short])).all() for k in whole), (short, with_index)
            assert part_index is None or (part_index == index[:short]).all()


NAMES = ("means3D", "shs", "opacities", "scales", "rotations")
LRS = dict(means3D=5e-4, shs=2e-3, opacities=5e-3, scales=5e-4, rotations=5e-4)


def _settings(views, W, H, sh_degree, dev):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=v["tanfovx"], tanfovy=v["tanfovy"], bg=torch.zeros(3, device=dev), scale_modifier=1.0,
        viewmatrix=v["viewmatrix"].to(dev), projmatrix=v["projmatrix"].to(dev), sh_degree=sh_degree, campos=v["campos"].to(dev),
        prefiltered=False, debug=False) for v in views]


def _render(params, settings, stats=None):
    import diff_gaussian_rasterization as d
    means2D = torch.zeros_like(params["means3D"], requires_grad=True)
    kw = dict(shs=params["shs"], scales=params["scales"], rotations=params["rotations"])
    if stats is None:
        return d.rasterize_views(params["means3D"], means2D, params["opacities"], settings, **kw)
    return d.rasterize_views_stats(params["means3D"], means2D, params["opacities"], settings, stats, **kw)


def _steps(params, opt, settings, target, stats, n):
    from pcrender import losses
    seen = []
    for _ in range(n):
        frames, radii = _render(params, settings, stats)
        loss = losses.photometric_loss(frames, target, 0.2).sum()
        loss.backward()
        seen.append(float(loss.detach()))
        opt.step(radii=radii, zero_grads=True)
    return seen


def test_training_loop_with_densify_and_prune(N, dev):
    import diff_gaussian_rasterization as d
    from pcrender import density, optim
    g, views, W, H = NC.cloud_views(4, P=3000, W=64, H=64)
    settings = _settings(views, W, H, g["sh_degree"], dev)
    rng = np.random.default_rng(8)
    with torch.no_grad():
        target, _ = _render({k: NC.to_device(g[k], dev) for k in NAMES}, settings)
    params = {k: NC.to_device(g[k] + 0.01 * rng.standard_normal(g[k].shape).astype(np.float32), dev).requires_grad_(True) for k in NAMES}
    P = params["means3D"].shape[0]
    opt = optim.GaussianAdam(params, LRS)
    stats = d.DensityStats(P, dev)
    first = _steps(params, opt, settings, target, stats, 10)
    host = lambda t: {k: v.detach().cpu().numpy().copy() for k, v in t.items()}  # noqa: E731
    old, h_stats = host(params), host(dict(g=stats.grad_norm_sum, v=stats.visible_views, r=stats.max_radius))
    # thresholds at quantiles of this cloud, so that every action occurs
    mean_grad = stats.mean_grad().cpu().numpy()
    smax = old["scales"].max(1)
    rule = density.DensityRule(grad_threshold=float(np.quantile(mean_grad, 0.6)), dense_size=float(np.median(smax)),
                               min_opacity=float(np.quantile(old["opacities"], 0.05)), max_screen_radius=max(1, int(np.quantile(h_stats["r"], 0.97))),
                               max_world_size=float(np.quantile(smax, 0.98)), seed=99)
    twin = optim.GaussianAdam({k: v.detach().clone().requires_grad_(True) for k, v in params.items()}, LRS)
    twin.load_state_dict(opt.state_dict())
    noise = torch.from_numpy(rng.standard_normal((P, 2, 3)).astype(np.float32)).to(dev)
    new_params, index = density.densify_and_prune(params, stats, rule, opt=opt, noise=noise)
    P2 = index.shape[0]
    s = rule.struct()
    ref_rule = R.make_rule(s.grad_threshold, s.dense_size, s.min_opacity, s.max_screen_radius, s.max_world_size, 0, 1, 99)
    action = R.actions(ref_rule, old["scales"], old["opacities"], h_stats["g"], h_stats["v"], h_stats["r"])
    assert (np.bincount(action, minlength=5)[[R.PRUNED, R.KEPT, R.CLONED, R.SPLIT]] > 0).all(), np.bincount(action, minlength=5)
    roles = dict(means3D=R.MEANS, scales=R.SCALES)
    want, want_index = R.apply_ref(ref_rule, action, [(old[k].reshape(P, -1), roles.get(k, R.COPY)) for k in NAMES], old["scales"],
                                   old["rotations"], noise.cpu().numpy())
    assert P2 == len(want_index) != P and (index.cpu().numpy() == want_index).all() and index.dtype == torch.int32
    assert opt.P == P2 and all(opt.params[k] is new_params[k] and new_params[k].requires_grad and new_params[k].is_leaf for k in NAMES)
    # the optimizer's moments are what reindex gives on a copy, bit for bit
    twin.reindex(index, {k: v.detach().clone().requires_grad_(True) for k, v in new_params.items()})
    for k in NAMES:
        assert torch.equal(opt.exp_avg[k].view(torch.int32), twin.exp_avg[k].view(torch.int32)), k
        assert torch.equal(opt.exp_avg_sq[k].view(torch.int32), twin.exp_avg_sq[k].view(torch.int32)), k
        assert opt.exp_avg[k].shape == new_params[k].shape
    # a render of the new cloud equals a render of the cloud the restatement builds from the same noise, bit for bit
    rebuilt = {k: NC.to_device(w.reshape((P2,) + old[k].shape[1:]), dev) for k, w in zip(NAMES, want)}
    with torch.no_grad():
        a, radii_a = _render(new_params, settings)
        b, radii_b = _render(rebuilt, settings)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(radii_a, radii_b) and a.abs().sum() > 0
    for k in NAMES:
        assert (_bits(new_params[k].detach().cpu().numpy()) == _bits(rebuilt[k].cpu().numpy())).all(), k
    # ten more steps on the new cloud: the loss falls
    second = _steps(new_params, opt, settings, target, d.DensityStats(P2, dev), 10)
    print("summed loss per iteration: %s | %s" % (" ".join("%.5f" % x for x in first), " ".join("%.5f" % x for x in second)))
    assert opt.t == 20 and first[-1] < first[0] and second[-1] < second[0]
