"""What the fused photometric loss (gsr_image_loss_forward + gsr_image_loss_backward) costs next to the torch float32 formulation of the
same loss -- grouped conv2d with the 121-tap window, avg_pool2d at rate 2, autograd -- in ONE process, and how accurate it is.

    python scripts/image_loss_cost.py [--rounds 12] [--warmup 3] [--views 12] [--out profiles/r23_image_loss.txt]

Two shapes: 12 views of 1920 x 1080 at ss = 1, and 12 views of 1024 x 1024 at ss = 2 (frames of 2048 x 2048).  A round is one forward
plus backward of each formulation, alternating, each between two device events on the current stream; the rounds follow a garbage
collection and benchlib.timing's untimed recovery load.  Reported per shape: median (min .. max) ms per call of both, their ratio, the
fused time against the byte model of 96 B per loss pixel at the bandwidth benchlib.roofline takes as achievable, the bytes the kernels
as written move, and the split between the two entries from gsr_get_profile (rounds of their own, after the timed ones).  Then the
accuracy figures of every case of tests/image_loss_ref.CASES: the gradient error e against float64, the float32 formulation's e32, and
their ratio."""
import argparse
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-pcloud-render_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

MODEL_BYTES_PER_PIXEL = 96


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    import torch
    from benchlib import roofline, timing
    from diff_gaussian_rasterization import _native as N
    import image_loss_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("image_loss_cost.py measures on the GPU: no HIP device is visible")
    dev = torch.device("cuda:0")
    V, lam = a.views, 0.2
    say("fused photometric loss against the torch float32 formulation, forward + backward, %d views per call; %s"
        % (V, N.lib.gsr_version().decode()))
    worst = None
    for W, H, ss in ((1920, 1080, 1), (1024, 1024, 2)):
        g = torch.Generator(device=dev).manual_seed(W + ss)
        image = torch.rand((V, 3, H * ss, W * ss), device=dev, generator=g)
        target = torch.rand((V, 3, H, W), device=dev, generator=g)
        state = N.image_loss_state(V, W, H, dev)
        grad = torch.empty_like(image)
        leaf = image.clone().requires_grad_(True)

        def fused():
            terms = N.image_loss_forward(image, target, lam, ss, state=state)
            N.image_loss_backward(image, target, lam, ss, state, out=grad)
            return terms

        def formulation():
            leaf.grad = None
            terms = R.loss_terms(leaf, target, lam, ss)
            terms[:, 3].sum().backward()
            return terms

        for _ in range(a.warmup):
            t_f, t_t = fused(), formulation()
        torch.cuda.synchronize()
        # faster and different is not faster: the two agree on what they time
        d_terms = float((t_f - t_t.detach()).abs().max())
        d_grad = float((grad - leaf.grad).abs().max() / leaf.grad.abs().max())
        gc.collect()
        end = time.perf_counter() + timing.GC_RECOVER_S
        while time.perf_counter() < end:
            fused()
        torch.cuda.synchronize()
        base = torch.cuda.Event(enable_timing=True)
        base.record()
        marks = {"fused": [], "torch": []}
        for _ in range(a.rounds):
            for name, fn in (("fused", fused), ("torch", formulation)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                marks[name].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: [x.elapsed_time(y) for x, y in v] for k, v in marks.items()}
        busy = {k: timing.union_ms([(base.elapsed_time(x), base.elapsed_time(y)) for x, y in v]) for k, v in marks.items()}
        med = {k: statistics.median(v) for k, v in ms.items()}
        ratio = med["torch"] / med["fused"]
        worst = ratio if worst is None else min(worst, ratio)
        pixels = V * H * W
        model_ms = MODEL_BYTES_PER_PIXEL * pixels / (roofline.HBM_ACHIEVABLE_GBS * 1e9) * 1e3
        # the kernels as written, per loss pixel and channel: forward reads x (ss^2 values) and y and writes A B C; backward reads
        # A B C, x and y and writes ss^2 gradients; halo re-reads (served by the caches) not counted
        written = 3 * 4 * ((ss * ss + 1 + 3) + (3 + ss * ss + 1 + ss * ss)) * pixels
        say()
        say("%d views, loss at %d x %d, ss = %d (frames %d x %d): ms per call, median (min .. max) of %d alternating rounds after %d warm-up "
            "rounds" % (V, W, H, ss, W * ss, H * ss, a.rounds, a.warmup))
        for k, label in (("fused", "fused entries (HIP)"), ("torch", "torch float32 formulation")):
            say("  %-28s %8.3f  (%.3f .. %.3f)   busy %.3f ms over the %d rounds" % (label, med[k], min(ms[k]), max(ms[k]), busy[k], a.rounds))
        say("  ratio torch / fused          %8.2f x   (required: at least 2)%s" % (ratio, "" if ratio >= 2 else "   BELOW THE REQUIRED 2 x"))
        say("  byte model, %d B per loss pixel at %.0f GB/s: %.3f ms; the fused time is %.2f x the model (the model is %.0f %% of it)"
            % (MODEL_BYTES_PER_PIXEL, roofline.HBM_ACHIEVABLE_GBS, model_ms, med["fused"] / model_ms, 100 * model_ms / med["fused"]))
        say("  bytes the kernels as written move: %.2f GB = %.0f B per loss pixel: %.3f ms at that bandwidth, %.0f %% of the fused time"
            % (written / 1e9, written / pixels, written / (roofline.HBM_ACHIEVABLE_GBS * 1e9) * 1e3,
               100 * written / (roofline.HBM_ACHIEVABLE_GBS * 1e9) * 1e3 / med["fused"]))
        say("  agreement of the two on these inputs: max|terms difference| %.3g, max|gradient difference| / max|gradient| %.3g" % (d_terms, d_grad))
        N.set_profiling(1)
        try:
            split = {"image_loss_fwd": [], "image_loss_bwd": []}
            for _ in range(5):
                fused()
                torch.cuda.synchronize()
                for name, t in N.get_profile():
                    if name in split:
                        split[name].append(t)
        finally:
            N.set_profiling(0)
        say("  gsr_get_profile, median of 5 calls: " + ", ".join("%s %.3f ms" % (k, statistics.median(v)) for k, v in split.items()))
        t0 = time.perf_counter()
        m = N.image_loss_forward(image, target, lam, ss, state=None)
        torch.cuda.synchronize()
        say("  metrics-only forward (no state block, one workgroup per view): %.1f ms; same loss_terms bits: %s"
            % ((time.perf_counter() - t0) * 1e3, bool(torch.equal(m, fused()))))
        del image, target, state, grad, leaf
    say()
    say("accuracy of the gradient per case of tests/image_loss_ref.CASES (worst view): e = max|g - g64| / max|g64|, e32 the float32 torch "
        "formulation's on the CPU; bar: e <= max(4 e32, 64 2^-24 = %.3g)" % R.GRAD_FLOOR)
    for c in R.CASES:
        r = R.measure(N, c, dev)
        v = int(r["e"].argmax())
        say("  %-16s V=%d %3d x %-3d ss=%d lambda=%.1f %-9s  e %.3e  e32 %.3e  e / e32 %.3g   worst term error %.2e (float32 %.2e)"
            % (c.name, c.V, c.W, c.H, c.ss, c.lam, c.content, r["e"][v], r["e32"][v], r["e"][v] / max(r["e32"][v], 1e-300),
               r["term_err"].max(), r["term_err32"].max()))
    say("  (identical: the float64 gradient is rounding noise around 0 and the library's is exactly 0, so e = 1 whatever the noise)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if worst >= 2 else 1


if __name__ == "__main__":
    sys.exit(main())
