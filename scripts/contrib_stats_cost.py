"""What gsr_contrib_stats costs at the benchmark's shape, next to the forward render kernel whose lists it walks, in ONE process.

    python scripts/contrib_stats_cost.py [--calls 7] [--warmup 3] [--points 800000] [--views 12] [--out profiles/r19_contrib_stats.txt]

The headline cloud (synth-THuman-800K, training profile, SH degree 1), 12 views of 1920 x 1080 in one submission.  Every round is one
forward (need_backward = 0) and then the variants of the new entry on its arenas, alternating, under gsr_set_profiling(1): one hipEvent
pair around every stage.  Reported per stage: median (min .. max) over the rounds, ms per 12-view call, and the ratio to render_forward
of the same rounds.
  contrib_stats, DPP        the lane reduction the library runs: four DPP steps per row of 16 lanes + the row totals through v_readlane
  contrib_stats, shuffle    the same kernel with six __shfl_xor butterflies (GSR_CONTRIB_REDUCE=1)
  ..., weight_sum only      one output instead of four: what the other three statistics' atomics and the maximum cost
  ..., with a weight map    all four outputs with a [V,H,W] map of ones"""
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

    import torch
    from diff_gaussian_rasterization import _native as N
    import native_calls as NC
    if not torch.cuda.is_available():
        raise SystemExit("contrib_stats_cost.py measures on the GPU: no HIP device is visible")
    dev = torch.device("cuda:0")
    W, H, V, P = 1920, 1080, a.views, a.points
    g, views, _, _ = NC.circle_scene(V, P=P, W=W, H=H)
    args = NC.cloud_args(g, views, W, H, dev, (1.0, 1.0, 1.0))
    outs = dict(weight_sum=torch.zeros(P, device=dev), weight_max=torch.zeros(P, device=dev),
                pixel_count=torch.zeros(P, dtype=torch.int32, device=dev), dominant_count=torch.zeros(P, dtype=torch.int32, device=dev))
    ones = torch.ones((V, H, W), device=dev)
    variants = (("contrib_stats, DPP", "0", outs, None), ("contrib_stats, shuffle", "1", outs, None),
                ("contrib_stats, DPP, weight_sum only", "0", dict(weight_sum=outs["weight_sum"]), None),
                ("contrib_stats, DPP, with a weight map", "0", outs, ones))

    def contrib(run, reduce, o, weights):
        os.environ["GSR_CONTRIB_REDUCE"] = reduce
        N.contrib_stats(args[0], args[1], run[2], args[2], args[4], args[5], args[6], args[7], args[8], args[9], args[10], args[11], H, W,
                        args[14], args[15], args[16], run[3], run[4], run[5], accumulate=False, pixel_weights=weights, **o)

    def round_(profile):
        run = N.rasterize_gaussians_batch(*args, need_backward=False)
        out = {}
        if profile:
            torch.cuda.synchronize()
            out.update(dict(N.get_profile()))
        for name, reduce, o, weights in variants:
            contrib(run, reduce, o, weights)
            if profile:
                torch.cuda.synchronize()
                out[name] = dict(N.get_profile())["contrib_stats"]
        return out, run

    say("contribution statistics at the benchmark's shape: P = %d, SH degree %d, %d views, %d x %d, one submission; %s"
        % (P, g["sh_degree"], V, W, H, N.lib.gsr_version().decode()))
    try:
        for _ in range(a.warmup):
            round_(False)
        torch.cuda.synchronize()
        N.set_profiling(1)
        runs = []
        for _ in range(a.calls):
            prof, run = round_(True)
            runs.append(prof)
    finally:
        N.set_profiling(0)
        os.environ.pop("GSR_CONTRIB_REDUCE", None)
    pairs = N.last_list_pairs(V)
    say("longest per-view lists of the %d views: %d pairs; contributions counted: %d; Gaussians with one: %d of %d"
        % (V, pairs, int(outs["pixel_count"].sum(dtype=torch.int64)), int((outs["pixel_count"] > 0).sum()), P))
    say("gsr_set_profiling(1) stage times, ms per %d-view call: median (min .. max) of %d rounds after %d warm-up rounds" % (V, a.calls, a.warmup))
    med = {}
    for name in ("render_forward",) + tuple(v[0] for v in variants):
        xs = [r[name] for r in runs]
        med[name] = statistics.median(xs)
        say("  %-40s %.4f  (%.4f .. %.4f)   %.2f x render_forward" % (name, med[name], min(xs), max(xs), med[name] / med["render_forward"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
