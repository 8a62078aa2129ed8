"""The fused Adam step on the device (gsr_adam_step / gsr_visible_from_radii, pcrender.optim.GaussianAdam) against the definition in
float64 (adam_ref), on the smallest shapes at which the kernel can go wrong: the case table names them with the kernel's own constants.
Every array sits between guard rows, masked rows are compared with the inputs bit for bit, and the mask output is prefilled.
The capped grid and its multi-round loops -- what a training cloud runs -- need 8 M elements: adam_ref.CAP_CASES, one test each.

Single-step bars (adam_ref.check_step; EPS = 2^-24, none taken from the kernel's results):
    |m' - m64| <= 4 EPS (|b1 m| + |c1 g|),  |v' - v64| <= 5 EPS v64,  |p' - (p - u64)| <= EPS |p - u64| + 8 EPS |u64|
with u64 the float64 update formed from the returned float32 m', v' and the float32 constants.  Trajectory bar: after 100 steps
e = max|p - p64| / max|p64 - p0| per group is at most 4 E32, E32 the largest e of the float32 restatement over the 8 seeds (computed
here on the CPU; 4 for another order of the same roundings)."""
import numpy as np
import pytest
import torch

import adam_ref as R
import native_calls as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    from diff_gaussian_rasterization import _native
    return _native


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _check_case(c, out, inputs, vis, t, what):
    worst = np.zeros(3)
    for k, (got, inp) in enumerate(zip(out, inputs)):
        worst = np.maximum(worst, R.check_step(got[:3], inp, c.lrs[k], t, vis, what="%s group %d (width %d)" % (what, k, c.widths[k])))
    return worst


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_single_step_dense_and_masked_against_float64(N, dev, c):
    before = N.lib.gsr_d2h_count()
    worst, dense = np.zeros(3), {}
    for t in R.TS:                                                        # dense, every step count
        out, inputs, _ = R.run_library(N, c, dev, None, t)
        worst = np.maximum(worst, _check_case(c, out, inputs, None, t, "%s dense t=%d" % (c.name, t)))
        assert all(R.same_bits(o[3], i[1]) for o, i in zip(out, inputs))            # without the flag the gradients stay
        dense[t] = out
    for k, kind in enumerate(R.MASKS):                                    # every mask, the step counts in turn
        t = R.TS[k % len(R.TS)]
        out, inputs, vis = R.run_library(N, c, dev, kind, t)
        worst = np.maximum(worst, _check_case(c, out, inputs, vis, t, "%s %s t=%d" % (c.name, kind, t)))
        if kind == "ones":                                                # the all-ones mask is the dense call, bit for bit
            assert all(R.same_bits(a, b) for o, d in zip(out, dense[t]) for a, b in zip(o, d))
        if kind == "zeros":
            assert all(R.same_bits(o[j], i[s]) for o, i in zip(out, inputs) for j, s in ((0, 0), (1, 2), (2, 3)))
        # zero_grads: every gradient element exactly 0, masked rows included; p', m', v' as without the flag
        flag, _, _ = R.run_library(N, c, dev, kind, t, zero_grads=True)
        for o, f in zip(out, flag):
            assert not f[3].view(np.uint32).any() and all(R.same_bits(a, b) for a, b in zip(o[:3], f[:3])), (c.name, kind)
    flag, _, _ = R.run_library(N, c, dev, None, 1, zero_grads=True)
    for o, f in zip(dense[1], flag):
        assert not f[3].view(np.uint32).any() and all(R.same_bits(a, b) for a, b in zip(o[:3], f[:3])), c.name
    assert N.lib.gsr_d2h_count() == before
    print("%s: worst error / bar  m %.3f  v %.3f  p %.3f" % (c.name, *worst))


def test_zero_gradient_and_zero_moments_leave_the_parameter_bits(N, dev):
    for P, width in ((257, 3), (65, 48), (R.rows_of_a_block(1) + 1, 1)):
        p = torch.randn((P, width), device=dev)
        p[0, 0] = -0.0
        g, m, v = (torch.zeros((P, width), device=dev) for _ in range(3))
        p0 = p.clone()
        N.adam_step([(p, g, m, v, 1e-2)], 1, R.BETA1, R.BETA2, R.ADAM_EPS)
        assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and not m.any() and not v.any()


def test_bits_repeat_groups_and_row_ranges_are_independent(N, dev):
    before = N.lib.gsr_d2h_count()
    for name in ("8groups,P=257", "offset1,P=65"):
        c = R.case(name)
        for kind in (None, "random30"):
            whole, _, _ = R.run_library(N, c, dev, kind, 2)
            again, _, _ = R.run_library(N, c, dev, kind, 2)
            assert all(R.same_bits(a, b) for o, d in zip(whole, again) for a, b in zip(o, d))       # two identical calls
            for k in range(len(c.widths)):                                                          # every group alone
                alone, inputs, _ = R.run_library(N, c, dev, kind, 2, only=(k,))
                assert all(R.same_bits(a, b) for a, b in zip(alone[k], whole[k])), (name, kind, k)
                other = (k + 1) % len(c.widths)                                                     # ... and nothing else was touched
                assert all(R.same_bits(alone[other][j], inputs[other][s]) for j, s in ((0, 0), (1, 2), (2, 3), (3, 1)))
            for a, b in ((5, c.P - 2), (1, 2), (c.P - 3, c.P)):                                     # rows [a, b) alone, a % 4 != 0
                assert a % R.VEC != 0
                part, inputs, _ = R.run_library(N, c, dev, kind, 2, rows=(a, b))
                for k in range(len(c.widths)):
                    assert all(R.same_bits(x[a:b], y[a:b]) for x, y in zip(part[k], whole[k])), (name, kind, k, a, b)
                    for j, s in ((0, 0), (1, 2), (2, 3), (3, 1)):                                   # the rows around them stay
                        assert R.same_bits(part[k][j][:a], inputs[k][s][:a]) and R.same_bits(part[k][j][b:], inputs[k][s][b:])
    assert N.lib.gsr_d2h_count() == before


@pytest.mark.parametrize("V", [1, 3, 12])
@pytest.mark.parametrize("P", [1, 63, 65, 1025])
def test_visible_from_radii_is_exact(N, dev, V, P):
    rng = np.random.default_rng(100 * V + P)
    radii = rng.choice(np.array([-7, -1, 0, 0, 0, 0, 0, 0, 0, 1, 2, 300], np.int32), (V, P))
    radii[:, P // 2] = 0
    radii[V - 1, P // 2] = 9                      # a column that is positive in the last view alone
    if P > 1:
        radii[:, 0] = -5                          # ... and one that is negative in every view
    want = (radii > 0).any(0)
    r = torch.from_numpy(radii).to(dev)
    out = torch.full((P + 2,), 255, dtype=torch.uint8, device=dev)
    got = N.visible_from_radii(r, out=out[1:P + 1])
    assert got.data_ptr() == out[1:].data_ptr() and out[0] == 255 and out[P + 1] == 255
    assert (got.cpu().numpy() == want.astype(np.uint8)).all()             # every element written: 0 or 1, never the prefill
    assert (N.visible_from_radii(r).cpu().numpy() == want.astype(np.uint8)).all()
    if V == 1:                                                            # the [P] radii of a single-view call
        assert (N.visible_from_radii(r[0].contiguous()).cpu().numpy() == want.astype(np.uint8)).all()


def _gradients_as_the_flag_says(out, inputs, flag, what):
    for o, i in zip(out, inputs):          # exactly 0 under zero_grads, the input's bits without it
        assert (not o[3].view(np.uint32).any()) if flag else R.same_bits(o[3], i[1]), what


CAP_RUNS = ((None, 1, False), ("random30", 3, True))     # mask kind, step count, zero_grads


@pytest.mark.parametrize("c", R.CAP_CASES, ids=[c.name for c in R.CAP_CASES])
def test_above_the_grid_cap_every_element_against_float64(N, dev, c):
    """More rounds than ADAM_MAX_BLOCKS (adam_ref.cap_cases says what each case reaches): a capped grid, floor-divided shares and
    workgroups that walk a second round -- what every call on a training cloud runs.  EVERY element is held to the single-step bars:
    a round that is skipped or taken twice shows in its own elements alone."""
    assert R.work_split(c.P, c.widths)[0] > R.MAX_BLOCKS
    before = N.lib.gsr_d2h_count()
    for kind, t, flag in CAP_RUNS:
        what = "%s %s t=%d" % (c.name, kind or "dense", t)
        out, inputs, vis = R.run_library(N, c, dev, kind, t, zero_grads=flag)     # (asserts that the guard rows are intact)
        worst = np.zeros(3)
        for k, (got, inp) in enumerate(zip(out, inputs)):
            worst = np.maximum(worst, R.check_step_in_ranges(got[:3], inp, c.lrs[k], t, vis, "%s group %d (width %d)" % (what, k, c.widths[k])))
        _gradients_as_the_flag_says(out, inputs, flag, what)
        print("%s: worst error / bar  m %.3f  v %.3f  p %.3f" % (what, *worst))
    assert N.lib.gsr_d2h_count() == before
    torch.cuda.empty_cache()               # (the case's 140 MB blocks go back: the tests after this one find the allocator as before)


def test_the_cloud_above_the_cap_in_two_halves_below_it_carries_the_same_bits(N, dev):
    """neither the workgroup nor the path enters a result: the rows of cap,cloud submitted as two calls, each below the cap and the
    second from a row that is no multiple of 4 (its width-3 and width-1 groups lose their alignment), against the one call"""
    c = R.case("cap,cloud")
    kind, t, flag = CAP_RUNS[1]
    whole, inputs, _ = R.run_library(N, c, dev, kind, t, zero_grads=flag)
    for a, b in R.CAP_CLOUD_HALVES:
        part, _, _ = R.run_library(N, c, dev, kind, t, zero_grads=flag, rows=(a, b))
        for k in range(len(c.widths)):
            assert all(R.same_bits(x[a:b], y[a:b]) for x, y in zip(part[k], whole[k])), (k, a, b)
            for j, s in ((0, 0), (1, 2), (2, 3), (3, 1)):                                           # the other half stays
                assert R.same_bits(part[k][j][:a], inputs[k][s][:a]) and R.same_bits(part[k][j][b:], inputs[k][s][b:]), (k, a, b)
    torch.cuda.empty_cache()


def test_visible_from_radii_past_its_grid_cap(N, dev):
    """one Gaussian more than ADAM_MAX_BLOCKS workgroups have lanes: the kernel's stride loop runs a second round, for the last one"""
    V, P = 2, R.VISIBLE_CAP_P
    rng = np.random.default_rng(100 * V + 7)
    radii = rng.choice(np.array([-7, -1, 0, 0, 0, 0, 0, 0, 0, 1, 2, 300], np.int32), (V, P))
    radii[:, P - 1] = 0
    radii[V - 1, P - 1] = 9                       # the last Gaussian is positive in the last view alone
    radii[:, 0] = -5
    want = (radii > 0).any(0)
    assert want[P - 1] and not want[0] and 0.3 < want.mean() < 0.7
    r = torch.from_numpy(radii).to(dev)
    out = torch.full((P + 2,), 255, dtype=torch.uint8, device=dev)
    got = N.visible_from_radii(r, out=out[1:P + 1])
    assert got.data_ptr() == out[1:].data_ptr() and out[0] == 255 and out[P + 1] == 255
    assert (got.cpu().numpy() == want.astype(np.uint8)).all()             # every element written: 0 or 1, never the prefill
    del r, out, got
    torch.cuda.empty_cache()


def _device_trajectory(N, dev, q, masked):
    """the library's own path: float32 on the device, gradients from the parameters it has reached"""
    p = [torch.from_numpy(a.copy()).to(dev) for a in q.p0]
    k, c = [torch.from_numpy(a).to(dev) for a in q.k], [torch.from_numpy(a).to(dev) for a in q.c]
    m, v = [torch.zeros_like(a) for a in p], [torch.zeros_like(a) for a in p]
    masks = torch.from_numpy(q.masks).to(dev)
    for t in range(1, R.TRAJ_STEPS + 1):
        groups = [(p[i], k[i] * (p[i] - c[i]), m[i], v[i], R.TRAJ_LRS[i]) for i in range(len(p))]
        N.adam_step(groups, t, R.BETA1, R.BETA2, R.ADAM_EPS, visible=masks[t - 1] if masked else None)
    return [a.cpu().numpy() for a in p]


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masked"])
def test_trajectory_of_100_steps_stays_with_float64(N, dev, masked):
    G = len(R.TRAJ_WIDTHS)
    e32, e = np.zeros((len(R.TRAJ_SEEDS), G)), np.zeros((len(R.TRAJ_SEEDS), G))
    for s, seed in enumerate(R.TRAJ_SEEDS):
        q = R.Quadratic(seed)
        p64, p32 = q.run(R.adam64, np.float64, masked), q.run(R.adam32, np.float32, masked)
        got = _device_trajectory(N, dev, q, masked)
        for i in range(G):
            e32[s, i], e[s, i] = R.trajectory_error(p32[i], p64[i], q.p0[i]), R.trajectory_error(got[i], p64[i], q.p0[i])
    E32 = e32.max(axis=0)
    print("%s: E32 per group %s;  e / E32 per seed and group:\n%s" % ("masked" if masked else "dense", E32, e / E32))
    assert (E32 > 0).all() and np.isfinite(e).all()
    assert (e <= 4 * E32).all(), (e / E32).max()


def test_offsets_past_four_gigabytes(N, dev):
    """One group whose four arrays lie more than 2^32 bytes into a single allocation (a P * width near 2^31 is too large for a test of
    seconds): its rows have to equal the same rows in a small allocation, bit for bit."""
    c = R.case("w45,P=257")
    n = c.P * 45
    stride = (n + 3) // 4 * 4 + 4
    big = torch.empty((1 << 30) + 16 + 4 * stride, dtype=torch.float32, device=dev)
    inputs = R.case_inputs(c)[0]
    vis = torch.from_numpy(R.mask("random30", c.P)).to(dev)
    for base in ((1 << 30) + 8, (1 << 30) + 9):                           # elements: 16-byte aligned (the dwordx4 path), then not
        far = [big[base + j * stride:base + j * stride + n].view(c.P, 45) for j in range(4)]
        near = [torch.from_numpy(a.copy()).to(dev) for a in inputs]
        for f, a in zip(far, near):
            f.copy_(a)
        assert all(f.data_ptr() - big.data_ptr() > 2 ** 32 for f in far) and (far[0].data_ptr() % 16 == 0) == (base % 4 == 0)
        for tensors in (far, near):
            N.adam_step([tuple(tensors) + (c.lrs[0],)], 3, R.BETA1, R.BETA2, R.ADAM_EPS, visible=vis, zero_grads=True)
        for f, a in zip(far, near):
            assert torch.equal(f.view(torch.int32), a.view(torch.int32)), base
        R.check_step(tuple(near[j].cpu().numpy() for j in (0, 2, 3)), inputs, c.lrs[0], 3, vis.cpu().numpy(), what="offsets")
    del big, far
    torch.cuda.empty_cache()


def _settings(views, W, H, sh_degree, dev):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=v["tanfovx"], tanfovy=v["tanfovy"], bg=torch.zeros(3, device=dev), scale_modifier=1.0,
        viewmatrix=v["viewmatrix"].to(dev), projmatrix=v["projmatrix"].to(dev), sh_degree=sh_degree, campos=v["campos"].to(dev),
        prefiltered=False, debug=False) for v in views]


NAMES = ("means3D", "shs", "opacities", "scales", "rotations")
HIDDEN = 300
CLOUD_LRS = dict(means3D=5e-4, shs=2e-3, opacities=5e-3, scales=5e-4, rotations=5e-4)


def _cloud(dev, jitter=0.0):
    """the synthetic cloud under three of the circle cameras; its last HIDDEN Gaussians are moved 50 units along the circle's axis, a
    right angle away from every camera's viewing direction, where no view sees them"""
    g, views, W, H = NC.cloud_views(3, P=3000, W=64, H=48)
    rng = np.random.default_rng(8)
    g = dict(g, means3D=g["means3D"].copy())
    axis = np.cross(views[0]["campos"].numpy().astype(np.float64), views[1]["campos"].numpy().astype(np.float64))
    g["means3D"][-HIDDEN:] = (50.0 * axis / np.linalg.norm(axis) + 0.1 * rng.standard_normal((HIDDEN, 3))).astype(np.float32)
    params = {k: torch.from_numpy(np.ascontiguousarray(g[k] + jitter * rng.standard_normal(g[k].shape).astype(np.float32))).to(dev)
              for k in NAMES}
    return params, _settings(views, W, H, g["sh_degree"], dev)


def _render(params, settings):
    import diff_gaussian_rasterization as d
    means2D = torch.zeros_like(params["means3D"], requires_grad=True)
    return d.rasterize_views(params["means3D"], means2D, params["opacities"], settings, shs=params["shs"], scales=params["scales"],
                             rotations=params["rotations"])


def test_one_iteration_through_the_optimizer_class_then_ten_then_reindex(N, dev):
    from pcrender import losses, optim
    target_params, settings = _cloud(dev, jitter=0.01)
    with torch.no_grad():
        target, _ = _render(target_params, settings)
    start, _ = _cloud(dev)
    params = {k: v.clone().requires_grad_(True) for k, v in start.items()}
    opt = optim.GaussianAdam(params, CLOUD_LRS)
    host = lambda d: {k: v.detach().cpu().numpy().copy() for k, v in d.items()}  # noqa: E731
    losses_seen = []
    for it in range(11):
        frames, radii = _render(params, settings)
        loss = losses.photometric_loss(frames, target, 0.2).sum()
        loss.backward()
        losses_seen.append(float(loss.detach()))
        if it == 0:          # the first iteration against the restatement, fed the same gradients and the mask of the radii
            assert tuple(frames.shape) == (3, 3, 48, 64) and tuple(radii.shape) == (3, 3000) and radii.dtype == torch.int32
            p0, g0, state0 = host(params), host({k: p.grad for k, p in params.items()}), opt.state_dict()
            vis = (radii > 0).any(0).cpu().numpy()
            assert vis[:-HIDDEN].sum() > 1000 and not vis[-HIDDEN:].any(), "the cloud has to have both seen and unseen Gaussians"
            before = N.lib.gsr_d2h_count()
            opt.step(radii=radii)
            assert N.lib.gsr_d2h_count() == before and opt.t == 1
            assert (opt._visible.cpu().numpy() == vis.astype(np.uint8)).all()
            p1, m1, v1 = host(params), host(opt.exp_avg), host(opt.exp_avg_sq)
            for k in NAMES:
                flat = lambda a: a.reshape(3000, -1)  # noqa: E731
                inp = (flat(p0[k]), flat(g0[k]), flat(state0["exp_avg"][k].cpu().numpy()), flat(state0["exp_avg_sq"][k].cpu().numpy()))
                R.check_step((flat(p1[k]), flat(m1[k]), flat(v1[k])), inp, CLOUD_LRS[k], 1, vis, what="GaussianAdam " + k)
                assert R.same_bits(flat(p1[k])[~vis], flat(p0[k])[~vis]) and not flat(m1[k])[~vis].any()     # rows no view saw
                assert (flat(p1[k])[vis] != flat(p0[k])[vis]).any()
                assert R.same_bits(host({k: params[k].grad})[k], g0[k])                                    # no zero_grads: kept
            for p in params.values():
                p.grad = None
        else:
            opt.step(radii=radii, zero_grads=True)
            assert all(not p.grad.any() for p in params.values())
    print("summed loss per iteration: %s" % " ".join("%.5f" % x for x in losses_seen))
    assert opt.t == 11 and losses_seen[-1] < losses_seen[0]

    # reindex: kept, duplicated and new (-1) rows, then a step against the restatement run on the reindexed float64 state
    rng = np.random.default_rng(5)
    index = np.concatenate([np.arange(0, 3000, 2), rng.integers(0, 3000, 700), np.full(300, -1)]).astype(np.int64)
    rng.shuffle(index)
    P2 = index.size
    src = np.clip(index, 0, None)
    m_old, v_old = host(opt.exp_avg), host(opt.exp_avg_sq)
    new_params = {k: params[k].detach()[torch.from_numpy(src).to(dev)].clone().requires_grad_(True) for k in NAMES}
    opt.reindex(torch.from_numpy(index).to(dev), new_params)
    assert opt.P == P2 and opt.t == 11
    grads = {k: torch.from_numpy(R.case_inputs(R.Case("reindex", P2, (new_params[k][0].numel(),), (1.0,), 0))[0][1]).to(dev)
             for k in NAMES}
    vis = R.mask("random30", P2)
    for k in NAMES:
        new_params[k].grad = grads[k].view_as(new_params[k]).clone()
    p0 = host(new_params)
    opt.step(visible=torch.from_numpy(vis).to(dev))
    for k in NAMES:
        flat = lambda a: np.ascontiguousarray(a.reshape(a.shape[0], -1))  # noqa: E731
        keep = (index >= 0)[:, None]
        inp = (flat(p0[k]), grads[k].cpu().numpy(), np.where(keep, flat(m_old[k])[src], 0).astype(np.float32),
               np.where(keep, flat(v_old[k])[src], 0).astype(np.float32))
        got = (flat(new_params[k].detach().cpu().numpy()), flat(opt.exp_avg[k].cpu().numpy()), flat(opt.exp_avg_sq[k].cpu().numpy()))
        R.check_step(got, inp, CLOUD_LRS[k], 12, vis, what="after reindex " + k)
