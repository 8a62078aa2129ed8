"""Cost of the deterministic colour backward (gsr_backward_batch_det) against the atomic backward of the same build, per stage
(gsr_set_profiling): the headline shape (12 views, 800 K points, 1920 x 1080) and a single view.

    python scripts/det_backward_cost.py [--points 800000] [--repeats 10] [--out profiles/r08_deterministic_backward_cost.txt]

Prints, per shape, the best-of-repeats ms of every stage of both backwards, the sums, and the scratch bytes."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-pcloud-render_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=800_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from diff_gaussian_rasterization import _native as N
    import native_calls as NC
    dev = torch.device("cuda:0")
    W, H = 1920, 1080
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for V in (12, 1):
        g, views, _, _ = NC.circle_scene(V, P=a.points, W=W, H=H)
        args = NC.cloud_args(g, views, W, H, dev, (0.0, 0.0, 0.0))
        run = N.rasterize_gaussians_batch(*args, need_backward=True)
        run = N.rasterize_gaussians_batch(*args, need_backward=True)      # (the second call's arena is sized from the first's counts)
        counts, color, radii, geom, binning, img = run
        pairs = N.last_list_pairs(V)
        need = N.query("TILE_NEED", a.points, W, H, 0, geom, binning, img, view=0, n_views=V).cpu().numpy().view(np.uint32)
        dpix = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (V, 3, H, W)).astype(np.float32)).to(dev)
        say("V = %d, P = %d, %d x %d: %d list pairs per view (max), %d consumed entries in view 0, scratch %.3f GB (%d bytes)" % (
            V, a.points, W, H, pairs, int(need.sum()), N.lib.gsr_backward_det_bytes(V, a.points, W, H, pairs) / 1e9,
            N.lib.gsr_backward_det_bytes(V, a.points, W, H, pairs)))
        for det in (False, True):
            best = {}
            for r in range(a.repeats + 2):
                N.set_profiling(1)
                N.rasterize_gaussians_backward_batch(args[0], args[1], radii, args[2], args[4], args[5], args[6], args[7], args[8], args[9],
                                                     args[10], args[11], dpix, args[14], args[15], args[16], geom, binning, img, False,
                                                     deterministic=det, pairs=pairs)
                torch.cuda.synchronize()
                prof = N.get_profile()
                N.set_profiling(0)
                if r < 2:
                    continue
                for k, v in prof:
                    best[k] = min(best.get(k, 1e9), v)
            say("  %-13s %s   sum %.4f ms (%.4f ms per view)" % ("deterministic" if det else "atomic",
                                                               "  ".join("%s %.4f" % kv for kv in best.items()), sum(best.values()),
                                                               sum(best.values()) / V))
        del run, geom, binning, img
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
