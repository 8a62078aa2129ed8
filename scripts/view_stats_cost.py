"""What gsr_backward_view_stats costs at the benchmark's shape, next to the backward whose records it reads, in ONE process.

    python scripts/view_stats_cost.py [--calls 7] [--warmup 3] [--points 800000] [--views 12] [--out profiles/r18_view_stats.txt]

The headline cloud (synth-THuman-800K, training profile, SH degree 1), 12 views of 1920 x 1080 in one submission.  Every call is a
forward (need_backward = 1), the colour backward and then the two variants of the new entry, under gsr_set_profiling(1): one hipEvent
pair around every stage.  Reported per stage: median (min .. max) over the calls, ms per 12-view call.
  view_stats, statistics only   grad_norm_sum / visible_views / max_radius with accumulate = 1 (what a training step adds)
  view_stats, with all shares   the same plus dL_dmean2D_views, dL_dcolor_views, dL_dopacity_views
and the condition of the statistics-only variant: no longer than preprocess_backward of the same run (it reads a subset of that
kernel's bytes).  The traffic figures are computed from the shapes, not measured."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-pcloud-render_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=800_000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from diff_gaussian_rasterization import _native as N
    import native_calls as NC
    if not torch.cuda.is_available():
        raise SystemExit("view_stats_cost.py measures on the GPU: no HIP device is visible")
    dev = torch.device("cuda:0")
    W, H, V, P = 1920, 1080, a.views, a.points
    g, views, _, _ = NC.circle_scene(V, P=P, W=W, H=H)
    args = NC.cloud_args(g, views, W, H, dev, (1.0, 1.0, 1.0))
    dpix = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (V, 3, H, W)).astype(np.float32)).to(dev)
    stats = (torch.zeros(P, device=dev), torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev))
    shares = (torch.empty((V, P, 2), device=dev), torch.empty((V, P, 3), device=dev), torch.empty((V, P), device=dev))

    def view_stats(radii, geom, with_shares):
        return N.backward_view_stats(args[0], args[1], radii, args[2], args[4], args[5], args[6], args[7], args[8], args[9], args[10],
                                     args[11], H, W, args[14], args[15], args[16], geom, accumulate=True, grad_norm_sum=stats[0],
                                     visible_views=stats[1], max_radius=stats[2], _out=shares if with_shares else None)

    def call(profile):
        counts, color, radii, geom, binning, img = N.rasterize_gaussians_batch(*args, need_backward=True)
        N.rasterize_gaussians_backward_batch(args[0], args[1], radii, args[2], args[4], args[5], args[6], args[7], args[8], args[9],
                                             args[10], args[11], dpix, args[14], args[15], args[16], geom, binning, img, False,
                                             deterministic=False)
        out = {}
        if profile:
            torch.cuda.synchronize()
            out.update({n: ms for n, ms in N.get_profile()})
        view_stats(radii, geom, False)
        if profile:
            torch.cuda.synchronize()
            out["view_stats, statistics only"] = dict(N.get_profile())["view_stats"]
        view_stats(radii, geom, True)
        if profile:
            torch.cuda.synchronize()
            out["view_stats, with all shares"] = dict(N.get_profile())["view_stats"]
        return out, radii

    say("view statistics at the benchmark's shape: P = %d, SH degree %d, %d views, %d x %d, one submission; %s"
        % (P, g["sh_degree"], V, W, H, N.lib.gsr_version().decode()))
    for _ in range(a.warmup):
        call(False)
    torch.cuda.synchronize()
    N.set_profiling(1)
    try:
        runs = []
        for _ in range(a.calls):
            prof, radii = call(True)
            runs.append(prof)
    finally:
        N.set_profiling(0)
    say("visible (view, Gaussian) pairs: %d of %d" % (int((radii > 0).sum()), V * P))
    say("gsr_set_profiling(1) stage times, ms per %d-view call: median (min .. max) of %d calls after %d warm-up calls" % (V, a.calls, a.warmup))
    med = {}
    for name in ("render_backward", "preprocess_backward", "view_stats, statistics only", "view_stats, with all shares"):
        xs = [r[name] for r in runs]
        med[name] = statistics.median(xs)
        say("  %-30s %.4f  (%.4f .. %.4f)" % (name, med[name], min(xs), max(xs)))
    # bytes from the shapes: a 64-B record line and a radius per (view, Gaussian); 12 B of running values read and written per
    # Gaussian; the shares add 24 B per (view, Gaussian) of stores
    b_stats = V * P * (64 + 4) + P * 24
    b_shares = b_stats + V * P * 24
    say("traffic from the shapes: statistics only %.3f GB -> %.2f TB/s; with all shares %.3f GB -> %.2f TB/s"
        % (b_stats / 1e9, b_stats / 1e9 / med["view_stats, statistics only"], b_shares / 1e9, b_shares / 1e9 / med["view_stats, with all shares"]))
    s, pb = med["view_stats, statistics only"], med["preprocess_backward"]
    say("condition (statistics only <= preprocess_backward of the same run): %.4f %s %.4f ms -- %s"
        % (s, "<=" if s <= pb else ">", pb, "holds" if s <= pb else "MISSED by %.4f ms (%.0f %%)" % (s - pb, 100 * (s - pb) / pb)))
    say("after %d accumulated calls: grad_norm_sum max %.4g, visible_views max %d, max_radius max %d"
        % (2 * (a.calls + a.warmup), float(stats[0].max()), int(stats[1].max()), int(stats[2].max())))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
