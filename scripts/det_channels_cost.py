"""Cost of the deterministic channels backward (gsr_backward_batch_channels_det) against the atomic channels backward of the same
build (whose render kernels are, instruction for instruction, the parent commit's), stage by stage (gsr_set_profiling): the workload
of profiles/r07_channels_backward.txt -- synth-THuman-800K, training profile, 12 circle views, 1920 x 1080, eight extra channels in
the split layout (xyz + hit shared, a per-view quad) -- and a single view of it.

    python scripts/det_channels_cost.py [--points 800000] [--blocks 5] [--calls 4] [--power-scene "..."]
                                        [--out profiles/r13_det_channels_backward.txt]

One process; blocks of `calls` backwards alternate between the two paths over one forward; per stage the median over the blocks of
the block's median call.  Also prints the scratch bytes per pair and in total."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-pcloud-render_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

# stage names of gsr_set_profiling -> the table's columns
STAGES = (("bwd_items", "items"), ("det_prepare", "prefix + emit"), ("det_sort", "sort"), ("render_backward", "render backward"),
          ("det_reduce", "reduce (records)"), ("det_reduce_extra", "reduce (extras)"), ("det_viewsum", "view sum"),
          ("preprocess_backward", "per-Gaussian"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=800_000)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--power-scene", default=None, help="line recorded from tests/test_gpu_deterministic_channels.py's power-scene test")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from diff_gaussian_rasterization import _native as N
    from pcrender import camera, synth
    dev = torch.device("cuda:0")
    W, H = 1920, 1080
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    cloud = synth.make_cloud("synth-THuman-800K", seed=0, P=a.points)
    g = synth.make_gaussians(cloud, profile="training", seed=1)
    P = g["means3D"].shape[0]
    say("Deterministic channels backward: cost against the atomic channels backward (one GPU session, one process); %s"
        % N.lib.gsr_version().decode())
    say("Workload: synth-THuman-800K (%d points), training profile, circle views, %d x %d, SH degree %d, black background, nx = 8 in the "
        "split layout (extra_per_view = 2).  ms per backward CALL; blocks of %d calls alternate between the paths, median over %d "
        "blocks of the block's median." % (P, W, H, g["sh_degree"], a.calls, a.blocks))
    rng = np.random.default_rng(5)
    for V in (12, 1):
        views = camera.circle_views(V, fov_deg=45.0, width_px=W, height_px=H)
        e = torch.empty(0)
        vm = torch.stack([v["viewmatrix"] for v in views]).to(dev)
        pm = torch.stack([v["projmatrix"] for v in views]).to(dev)
        cp = torch.stack([v["campos"] for v in views]).to(dev)
        args = [t(np.zeros(3, np.float32)), t(g["means3D"]), e, t(g["opacities"]), t(g["scales"]), t(g["rotations"]), 1.0, e, vm, pm,
                views[0]["tanfovx"], views[0]["tanfovy"], H, W, t(g["shs"]), g["sh_degree"], cp, False, False]
        lo = torch.cat([args[1], torch.ones((P, 1), device=dev)], 1).contiguous()
        hi = t(rng.normal(0, 1, (V, P, 4)).astype(np.float32))
        extra = ((lo, hi), None, torch.zeros(8, device=dev))
        run = N.rasterize_gaussians_batch(*args, need_backward=True, extra=extra)
        del run
        run = N.rasterize_gaussians_batch(*args, need_backward=True, extra=extra)   # (the second call's arena is sized from the first's counts)
        counts, color, radii, geom, binning, img, out_x = run
        pairs = N.last_list_pairs(V)
        dpix = t(rng.uniform(-1, 1, (V, 3, H, W)).astype(np.float32))
        dx = t(rng.uniform(-1, 1, (V, 8, H, W)).astype(np.float32))
        total = int(N.lib.gsr_backward_det_channels_bytes(V, P, W, H, pairs, 8, 2))
        colour = int(N.lib.gsr_backward_det_bytes(V, P, W, H, pairs))
        say()
        say("V = %d: %d list pairs per view (max).  Scratch: %d bytes (%.3f GB) = %.1f bytes per pair and view + %d bytes of view staging "
            "(the colour entry's block: %.3f GB, %.1f bytes per pair and view)" % (
                V, pairs, total, total / 1e9, (total - 16 * V * P - 256) / (V * pairs), 16 * V * P, colour / 1e9, (colour - 256) / (V * pairs)))

        def block(det):
            per = {}
            for _ in range(a.calls):
                N.set_profiling(1)
                N.rasterize_gaussians_backward_channels_batch(args[0], args[1], radii, args[2], args[4], args[5], 1.0, args[7], args[8], args[9],
                                                              args[10], args[11], dpix, args[14], args[15], args[16], geom, binning, img,
                                                              False, extra, dx, deterministic=det, pairs=pairs)
                torch.cuda.synchronize()
                prof = N.get_profile()
                N.set_profiling(0)
                tot = {}
                for k, v in prof:
                    tot[k] = tot.get(k, 0.0) + v
                tot["sum"] = sum(tot.values())
                for k, v in tot.items():
                    per.setdefault(k, []).append(v)
            return {k: float(np.median(v)) for k, v in per.items()}

        block(False), block(True)                                    # warm-up: both paths, allocator included
        res = {False: [], True: []}
        for _ in range(a.blocks):
            for det in (False, True):
                res[det].append(block(det))
        med = {det: {k: float(np.median([b.get(k, 0.0) for b in res[det]])) for k in set().union(*res[det])} for det in res}
        say("  %-18s %10s %14s" % ("stage", "atomic", "deterministic"))
        for key, label in STAGES:
            say("  %-18s %10s %14s" % (label, "%.4f" % med[False][key] if key in med[False] else "-",
                                       "%.4f" % med[True][key] if key in med[True] else "-"))
        say("  %-18s %10.4f %14.4f   (%.2fx; %.4f / %.4f ms per view)" % ("sum of the stages", med[False]["sum"], med[True]["sum"],
                                                                        med[True]["sum"] / med[False]["sum"], med[False]["sum"] / V,
                                                                        med[True]["sum"] / V))
        other = sorted(set(med[True]) - {k for k, _ in STAGES} - {"sum"})
        if other:
            say("  (stages not in the table: %s)" % ", ".join("%s %.4f" % (k, med[True][k]) for k in other))
        del run, geom, binning, img, out_x, color, radii, hi, lo, extra, dpix, dx
        torch.cuda.empty_cache()
    if a.power_scene:
        say()
        say(a.power_scene)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
