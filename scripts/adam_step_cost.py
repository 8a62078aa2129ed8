"""What the fused Adam step (gsr_adam_step) costs next to torch.optim.Adam on the same tensors, in ONE process, dense and with
visibility masks.

    python scripts/adam_step_cost.py [--rounds 20] [--warmup 3] [--points 800000] [--out profiles/r24_adam_step.txt]

Workload: a cloud of P = 800 000 Gaussians with the five parameter groups of a degree-3 splat model -- widths 3 (means), 48 (SH), 1
(opacity), 3 (scales), 4 (rotations): 59 floats per Gaussian.  A round runs every variant once, alternating, each between two device
events on the current stream: the fused call dense, with random row masks of several visible fractions, and with the mask of a real
12-view batch of the benchmark's cloud (gsr_visible_from_radii of its radii); torch.optim.Adam(fused=True) and (foreach=True) on the
same shapes.  Reported: median (min .. max) ms per step, the multiple of the byte model -- 28 B per updated element (read p, g, m, v;
write p, m, v) plus the mask's P bytes, at the bandwidth benchlib.roofline takes as achievable --, the ratio to torch's fused Adam, and
the visible fraction below which the masked step is faster than the dense one.  The times are written down as they come out: no bar
is set on them."""
import argparse
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-pcloud-render_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

WIDTHS = (3, 48, 1, 3, 4)
LRS = (1.6e-4, 2.5e-3, 5e-2, 5e-3, 1e-3)
FRACTIONS = (1.0, 0.7, 0.5, 0.3, 0.1, 0.05)
MODEL_BYTES_PER_ELEMENT = 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=800_000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    import torch
    import diff_gaussian_rasterization as d
    from benchlib import roofline, timing
    from diff_gaussian_rasterization import _native as N
    from pcrender import camera, synth
    if not torch.cuda.is_available():
        raise SystemExit("adam_step_cost.py measures on the GPU: no HIP device is visible")
    dev = torch.device("cuda:0")
    P = a.points
    elements = P * sum(WIDTHS)
    say("fused Adam step against torch.optim.Adam, P = %d Gaussians, groups of width %s (%d floats each, %.1f M elements); %s"
        % (P, ", ".join(map(str, WIDTHS)), sum(WIDTHS), elements / 1e6, N.lib.gsr_version().decode()))

    # the mask of a real batch: the benchmark's cloud and circle cameras at 1080p, forward only
    cloud = synth.make_cloud("synth-THuman-800K", seed=0, P=P)
    g = synth.make_gaussians(cloud, profile="training", seed=1)
    views = camera.circle_views(n_imgs=a.views, fov_deg=45.0, width_px=1920, height_px=1080)
    settings = [d.GaussianRasterizationSettings(
        image_height=1080, image_width=1920, tanfovx=v["tanfovx"], tanfovy=v["tanfovy"], bg=torch.ones(3, device=dev), scale_modifier=1.0,
        viewmatrix=v["viewmatrix"].to(dev), projmatrix=v["projmatrix"].to(dev), sh_degree=g["sh_degree"], campos=v["campos"].to(dev),
        prefiltered=False, debug=False) for v in views]
    t = lambda k: torch.from_numpy(g[k]).to(dev)  # noqa: E731
    with torch.no_grad():
        means3D = t("means3D")
        _, radii = d.rasterize_views(means3D, torch.zeros_like(means3D), t("opacities"), settings, shs=t("shs"), scales=t("scales"),
                                     rotations=t("rotations"))
    batch_mask = N.visible_from_radii(radii)
    one_view_mask = N.visible_from_radii(radii[:1].contiguous())
    torch.cuda.synchronize()
    del means3D

    gen = torch.Generator(device=dev).manual_seed(24)
    rand = lambda w: torch.randn((P, w), device=dev, generator=gen)  # noqa: E731
    params = [rand(w) for w in WIDTHS]
    grads = [rand(w) * 1e-3 for w in WIDTHS]
    m, v = [torch.zeros_like(x) for x in params], [torch.zeros_like(x) for x in params]
    groups = [(params[i], grads[i], m[i], v[i], LRS[i]) for i in range(len(WIDTHS))]
    order = torch.rand(P, device=dev, generator=gen)
    masks = {"random %3.0f %%" % (100 * f): (order < f).to(torch.uint8) for f in FRACTIONS}
    masks["%d-view batch" % a.views] = batch_mask
    masks["1-view batch"] = one_view_mask
    visible = {k: float(x.float().mean()) for k, x in masks.items()}
    step = [0]

    def fused(mask=None):
        step[0] += 1
        N.adam_step(groups, step[0], 0.9, 0.999, 1e-15, visible=mask)

    tparams = [torch.nn.Parameter(x.clone()) for x in params]
    for tp, gr in zip(tparams, grads):
        tp.grad = gr.clone()
    opts = {}
    for name, kw in (("torch fused=True", dict(fused=True)), ("torch foreach=True", dict(foreach=True))):
        opts[name] = torch.optim.Adam([dict(params=[tp], lr=lr) for tp, lr in zip(tparams, LRS)], betas=(0.9, 0.999), eps=1e-15, **kw)
    variants = [("fused HIP, dense", lambda: fused(None))]
    variants += [("fused HIP, " + k, (lambda x: lambda: fused(x))(x)) for k, x in masks.items()]
    variants += [(k, o.step) for k, o in opts.items()]
    variants.append(("visible_from_radii, %d views" % a.views, lambda: N.visible_from_radii(radii, out=batch_mask)))

    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    gc.collect()
    end = time.perf_counter() + timing.GC_RECOVER_S
    while time.perf_counter() < end:
        fused(None)
    torch.cuda.synchronize()
    marks = {k: [] for k, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            marks[name].append((e0, e1))
    torch.cuda.synchronize()
    ms = {k: [x.elapsed_time(y) for x, y in vv] for k, vv in marks.items()}
    med = {k: statistics.median(x) for k, x in ms.items()}
    bw = roofline.HBM_ACHIEVABLE_GBS * 1e9

    say()
    say("ms per step, median (min .. max) of %d alternating rounds after %d warm-up rounds; byte model: %d B per updated element (+ P "
        "mask bytes) at %.0f GB/s" % (a.rounds, a.warmup, MODEL_BYTES_PER_ELEMENT, roofline.HBM_ACHIEVABLE_GBS))
    say("  %-30s %8s %20s %9s %11s %14s" % ("variant", "visible", "ms", "model ms", "x model", "torch fused /"))
    ref = med["torch fused=True"]
    for name, _ in variants:
        if name.startswith("visible_from_radii"):
            model = (4 * a.views + 1) * P / bw * 1e3
            frac = ""
        elif name.startswith("fused HIP, ") and name != "fused HIP, dense":
            f = visible[name[len("fused HIP, "):]]
            model, frac = (MODEL_BYTES_PER_ELEMENT * elements * f + P) / bw * 1e3, "%.1f %%" % (100 * f)
        else:
            model, frac = MODEL_BYTES_PER_ELEMENT * elements / bw * 1e3, "100 %"
        say("  %-30s %8s %8.3f (%.3f .. %.3f) %9.3f %11.2f %14.2f"
            % (name, frac, med[name], min(ms[name]), max(ms[name]), model, med[name] / model, ref / med[name]))
    say()
    dense = med["fused HIP, dense"]
    say("dense fused step against torch: %.3f ms, torch fused=True %.3f ms (%.2f x), torch foreach=True %.3f ms (%.2f x): the dense step is %s "
        "torch's fused Adam" % (dense, ref, ref / dense, med["torch foreach=True"], med["torch foreach=True"] / dense,
                                "FASTER than" if dense < ref else "NOT faster than"))
    pays = [f for f in FRACTIONS if med["fused HIP, random %3.0f %%" % (100 * f)] < dense]
    say("masking (random rows) is faster than the dense step at visible fractions %s of those measured (%s)"
        % (", ".join("%.0f %%" % (100 * f) for f in pays) if pays else "none", ", ".join("%.0f %%" % (100 * f) for f in FRACTIONS)))
    say("the %d-view batch of the benchmark's cloud sees %.1f %% of the Gaussians, one view %.1f %%"
        % (a.views, 100 * visible["%d-view batch" % a.views], 100 * visible["1-view batch"]))
    # faster and different is not faster: one dense step of each from the same state agrees
    p0 = [x.clone() for x in params]
    chk = [torch.nn.Parameter(x.clone()) for x in p0]
    for tp, gr in zip(chk, grads):
        tp.grad = gr
    torch.optim.Adam([dict(params=[tp], lr=lr) for tp, lr in zip(chk, LRS)], betas=(0.9, 0.999), eps=1e-15, fused=True).step()
    mine = [(x.clone(), torch.zeros_like(x), torch.zeros_like(x)) for x in p0]
    N.adam_step([(pp, gr, mm, vv, lr) for (pp, mm, vv), gr, lr in zip(mine, grads, LRS)], 1, 0.9, 0.999, 1e-15)
    diff = max(float((pp - tp.detach()).abs().max() / (tp.detach() - x0).abs().max()) for (pp, _, _), tp, x0 in zip(mine, chk, p0))
    say("agreement on one dense step from the same state: max|p - p_torch| / max|update| = %.3g" % diff)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
