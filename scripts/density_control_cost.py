"""What adaptive density control in HIP (gsr_density_plan / gsr_density_apply, pcrender.density.densify_and_prune) costs next to the
torch formulation of the same step, in ONE process, alternating.

    python scripts/density_control_cost.py [--rounds 10] [--warmup 2] [--points 800000] [--out profiles/r25_density_control.txt]

Workload: the benchmark's cloud of P = 800 000 Gaussians with the five parameter groups of a degree-3 splat model -- widths 3 (means),
48 (SH; the benchmark's cloud renders with degree 1, its higher coefficients are zero), 1 (opacity), 3 (scales), 4 (rotations): 59
floats per Gaussian -- and the DensityStats that a few 12-view backward batches at 1080p leave.  Three synthetic regimes: the gradient
threshold is the quantile of the averaged gradient at which about 1 %, 10 % and 40 % of the Gaussians densify; dense_size is the median of the largest scale (half of them clone, half split), min_opacity 0.005, the
screen-radius threshold the 99.5 % quantile of the radii, the world-size threshold the 99.9 % quantile of the largest scale.

A round runs every variant once, each between two device events on the current stream: the plan (three launches); the apply of the
five parameter groups (index kernel + one gather); the apply of both moments (two calls); the whole densify_and_prune with the
optimizer (plan, the 8-byte read of P', allocation of the new leaves and moments, three applies, the hand-over); and the torch
formulation written out below: 3DGS's clone / split / prune with masks, cat, bmm and boolean indexing over every group, followed by
GaussianAdam.reindex.  The optimizer of the whole-step variants is rebuilt outside the timed window before every call (the step
changes its size).  Reported: median (min .. max) ms, and the multiple of the byte model at the bandwidth benchlib.roofline takes as
achievable: plan 28 B read + 5 B written per Gaussian (+ 1 with a mask); apply, per group, P x row bytes in + P' x row bytes out, + 4 P'
bytes of index written once and read once per group.  The times are written down as they come out: no bar is set on them."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-pcloud-render_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

NAMES = ("means3D", "shs", "opacities", "scales", "rotations")
LRS = dict(means3D=1.6e-4, shs=2.5e-3, opacities=5e-2, scales=5e-3, rotations=1e-3)
FRACTIONS = (0.01, 0.10, 0.40)


def torch_densify_and_prune(params, stats, rule, noise):
    """3DGS's densify_and_prune in torch on the library's tensors: (new_params, index), rows in 3DGS's order (kept, clones, children).
    index as GaussianAdam.reindex takes it: the source row of a carried row, -1 for a new one."""
    import torch
    P = params["means3D"].shape[0]
    cloud = {k: v.detach() for k, v in params.items()}
    index = torch.arange(P, device=noise.device)
    radii = stats.max_radius
    grads = stats.grad_norm_sum / stats.visible_views.clamp(min=1).to(torch.float32)
    grads[grads.isnan()] = 0.0
    # clone
    selected = (grads >= rule.grad_threshold) & (cloud["scales"].max(1).values <= rule.dense_size)
    n_clone = int(selected.sum())
    cloud = {k: torch.cat([v, v[selected]], 0) for k, v in cloud.items()}
    index = torch.cat([index, torch.full((n_clone,), -1, device=index.device)])
    radii = torch.cat([radii, torch.zeros(n_clone, dtype=radii.dtype, device=radii.device)])
    # split
    padded = torch.zeros(P + n_clone, device=grads.device)
    padded[:P] = grads
    selected = (padded >= rule.grad_threshold) & (cloud["scales"].max(1).values > rule.dense_size)
    n_split = int(selected.sum())
    stds = cloud["scales"][selected].repeat(2, 1)
    samples = torch.cat([noise[selected[:P]][:, 0], noise[selected[:P]][:, 1]], 0) * stds       # torch.normal(0, stds) with the given draws
    q = cloud["rotations"][selected]
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rots = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3).repeat(2, 1, 1)
    new = {k: v[selected].repeat(*([2] + [1] * (v.dim() - 1))) for k, v in cloud.items()}
    new["means3D"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + cloud["means3D"][selected].repeat(2, 1)
    new["scales"] = cloud["scales"][selected].repeat(2, 1) / (0.8 * 2)
    cloud = {k: torch.cat([v, new[k]], 0) for k, v in cloud.items()}
    index = torch.cat([index, torch.full((2 * n_split,), -1, device=index.device)])
    radii = torch.cat([radii, torch.zeros(2 * n_split, dtype=radii.dtype, device=radii.device)])
    keep = ~torch.cat([selected, torch.zeros(2 * n_split, dtype=torch.bool, device=selected.device)])
    cloud, index, radii = {k: v[keep] for k, v in cloud.items()}, index[keep], radii[keep]
    # prune
    prune = (cloud["opacities"] < rule.min_opacity).reshape(-1)
    if rule.max_screen_radius > 0:
        prune |= radii > rule.max_screen_radius
    if rule.max_world_size > 0:
        prune |= cloud["scales"].max(1).values > rule.max_world_size
    keep = ~prune
    return {k: v[keep].contiguous().requires_grad_(True) for k, v in cloud.items()}, index[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=800_000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    import diff_gaussian_rasterization as d
    from benchlib import roofline
    from diff_gaussian_rasterization import _native as N
    from pcrender import camera, density, losses, optim, synth
    if not torch.cuda.is_available():
        raise SystemExit("density_control_cost.py measures on the GPU: no HIP device is visible")
    dev = torch.device("cuda:0")
    P = a.points
    cloud = synth.make_cloud("synth-THuman-800K", seed=0, P=P)
    g = synth.make_gaussians(cloud, profile="training", seed=1)
    views = camera.circle_views(n_imgs=a.views, fov_deg=45.0, width_px=a.width, height_px=a.height)
    settings = [d.GaussianRasterizationSettings(
        image_height=a.height, image_width=a.width, tanfovx=v["tanfovx"], tanfovy=v["tanfovy"], bg=torch.ones(3, device=dev),
        scale_modifier=1.0, viewmatrix=v["viewmatrix"].to(dev), projmatrix=v["projmatrix"].to(dev), sh_degree=g["sh_degree"],
        campos=v["campos"].to(dev), prefiltered=False, debug=False) for v in views]
    params = {k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev).requires_grad_(True) for k in NAMES}
    say("adaptive density control in HIP against the torch formulation, P = %d Gaussians; %s" % (P, N.lib.gsr_version().decode()))

    # the statistics of a few backward batches of the benchmark's views against a slightly different cloud
    stats = d.DensityStats(P, dev)
    rng = np.random.default_rng(25)
    render = lambda ps, st=None: (d.rasterize_views if st is None else d.rasterize_views_stats)(  # noqa: E731
        ps["means3D"], torch.zeros_like(ps["means3D"], requires_grad=True), ps["opacities"], settings, *(() if st is None else (st,)),
        shs=ps["shs"], scales=ps["scales"], rotations=ps["rotations"])
    with torch.no_grad():
        target, _ = render({k: (v + 0.01 * torch.from_numpy(rng.standard_normal(v.shape).astype(np.float32)).to(dev)) if k == "shs" else v
                            for k, v in params.items()})
    for _ in range(a.batches):
        frames, _ = render(params, stats)
        losses.photometric_loss(frames, target, 0.2).sum().backward()
    for p in params.values():
        p.grad = None
    del frames, target
    # the benchmark's cloud carries SH degree 1; the timed cloud carries the 16 coefficients of degree 3 (the rest zero): 59 floats
    shs = torch.zeros((P, 16, 3), device=dev)
    shs[:, :params["shs"].shape[1]] = params["shs"].detach()
    params["shs"] = shs.requires_grad_(True)
    widths = {k: params[k][0].numel() for k in NAMES}
    row = sum(widths.values())
    torch.cuda.empty_cache()
    mean_grad = stats.mean_grad()
    smax = params["scales"].detach().max(1).values
    say("statistics of %d backward batches of %d views at %dx%d: %.1f %% of the Gaussians seen, averaged gradient median %.3g, radii up to %d"
        % (a.batches, a.views, a.width, a.height, 100 * float((stats.visible_views > 0).float().mean()), float(mean_grad.median()),
           int(stats.max_radius.max())))
    say("the timed cloud: %d floats per Gaussian (%s)" % (row, ", ".join("%s %d" % kv for kv in widths.items())))
    q = lambda t, f: float(torch.quantile(t.float()[:: max(1, t.numel() // 1_000_000)], f))  # noqa: E731
    noise = torch.randn((P, 2, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(25))
    gen = torch.Generator(device=dev).manual_seed(26)
    bw = roofline.HBM_ACHIEVABLE_GBS * 1e9

    def fresh_opt():
        opt = optim.GaussianAdam(params, LRS)
        for part in (opt.exp_avg, opt.exp_avg_sq):
            for k in part:
                part[k].normal_(generator=gen)
        return opt

    for f in FRACTIONS:
        rule = density.DensityRule(grad_threshold=q(mean_grad, 1.0 - f), dense_size=q(smax, 0.5), min_opacity=0.005,
                                   max_screen_radius=max(1, int(q(stats.max_radius, 0.995))), max_world_size=q(smax, 0.999), seed=25)
        pl = density.plan(params, stats, rule)
        P2, carried, copies, children, gone = pl.counts
        say()
        say("regime %.0f %%: grad_threshold %.3g -> P' = %d (%d carried, %d copies, %d children, %d Gaussians gone): %.1f %% densify"
            % (100 * f, rule.grad_threshold, P2, carried, copies, children, gone, 100.0 * (copies + children / 2) / P))
        new = {k: torch.empty((P2,) + tuple(v.shape[1:]), device=dev) for k, v in params.items()}
        index = torch.empty((P2,), dtype=torch.int32, device=dev)
        moments = [{k: torch.randn_like(v) for k, v in params.items()} for _ in range(2)]
        new_m = [{k: torch.empty_like(v) for k, v in new.items()} for _ in range(2)]
        roles = density.default_roles(NAMES)
        param_groups = [(params[k].detach(), new[k], density.ROLES[roles[k]]) for k in NAMES]
        geometry = dict(scales=params["scales"].detach(), rotations=params["rotations"].detach(), noise=noise)
        state = {}

        def run_plan():
            density.plan(params, stats, rule)

        def run_apply_params():
            N.density_apply(param_groups, pl.rule, pl.offsets, pl.action, P2, index=index, **geometry)

        def run_apply_moments():
            for src, dst in zip(moments, new_m):
                N.density_apply([(src[k], dst[k], N.DENSITY_MOMENT) for k in NAMES], pl.rule, pl.offsets, pl.action, P2, index=index)

        def run_whole():
            state["hip"] = density.densify_and_prune(params, stats, rule, opt=state["opt"], noise=noise)

        def run_torch():
            new_params, idx = torch_densify_and_prune(params, stats, rule, noise)
            state["opt"].reindex(idx, new_params)
            state["torch"] = (new_params, idx)

        variants = [("plan", run_plan, False), ("apply, parameters", run_apply_params, False), ("apply, both moments", run_apply_moments, False),
                    ("densify_and_prune with the optimizer", run_whole, True), ("torch formulation + reindex", run_torch, True)]
        ms = {k: [] for k, _, _ in variants}
        for r in range(a.warmup + a.rounds):
            for name, fn, needs_opt in variants:
                if needs_opt:
                    state["opt"] = fresh_opt()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        model = {"plan": 33.0 * P / bw * 1e3,
                 "apply, parameters": (4.0 * row * (P + P2) + 4.0 * P2 * (1 + len(NAMES))) / bw * 1e3}
        model["apply, both moments"] = 2 * model["apply, parameters"]
        model["densify_and_prune with the optimizer"] = model["plan"] + 3 * model["apply, parameters"]
        model["torch formulation + reindex"] = model["densify_and_prune with the optimizer"]
        say("  ms, median (min .. max) of %d alternating rounds after %d warm-up rounds; byte model at %.0f GB/s" % (a.rounds, a.warmup, bw / 1e9))
        say("  %-40s %24s %9s %9s" % ("variant", "ms", "model ms", "x model"))
        for name, _, _ in variants:
            m = statistics.median(ms[name])
            say("  %-40s %8.3f (%.3f .. %.3f) %9.3f %9.2f" % (name, m, min(ms[name]), max(ms[name]), model[name], m / model[name]))
        hip, ref = statistics.median(ms["densify_and_prune with the optimizer"]), statistics.median(ms["torch formulation + reindex"])
        say("  the whole step: HIP %.3f ms, torch %.3f ms (%.2f x): the HIP step is %s the torch formulation"
            % (hip, ref, ref / hip, "FASTER than" if hip < ref else "NOT faster than"))
        # faster and different is not faster: the same rows (the orders differ by design)
        (hp, hidx), (tp, tidx) = state["hip"], state["torch"]
        same_rows = hidx.shape[0] == tidx.shape[0]
        carried_h, carried_t = torch.sort(hidx[hidx >= 0]).values, torch.sort(tidx[tidx >= 0]).values
        same_rows = same_rows and torch.equal(carried_h.long(), carried_t.long())
        drift = max(float((torch.sort(hp[k].detach().reshape(hidx.shape[0], -1)[:, 0]).values -
                           torch.sort(tp[k].detach().reshape(tidx.shape[0], -1)[:, 0]).values).abs().max()) for k in NAMES) if same_rows else -1.0
        say("  agreement: P' %d / %d, the same carried rows: %s, largest difference of the sorted first columns of any group %.3g"
            % (hidx.shape[0], tidx.shape[0], same_rows, drift))
        del new, new_m, moments, state
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f_:
            f_.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
