"""What the fast arithmetic of TRAINING calls (gsr_set_train_math(1): the RenderFast forward kernels with their checkpoint stores and
the RenderBwdFast backward kernels) costs and buys against the exact mode of the same build, in ONE process: exact and fast blocks
ALTERNATE after a warm-up, every figure is the median over the blocks and the spread between blocks is printed next to it (a
difference inside the spread is no difference).

    python scripts/train_math_cost.py [--blocks 7] [--calls 5] [--cases 96] [--resources FILE] [--out profiles/r15_train_math.txt]
    python scripts/train_math_cost.py --resources-only          (no GPU: compiles render_bwd.hip for the device and prints the table)

Timing: the headline cloud (synth-THuman-800K, training profile, 1920 x 1080), forward (need_backward = 1) + backward, 12 views per call
and 1 view per call.  Per mode: the forward render kernel and the backward render kernel (gsr_set_profiling(2): one event pair around
each), with the atomic flush (gsr_backward_batch) and with the storing flush (gsr_backward_batch_det), and the whole forward + backward
call (device events around the block of calls), ms per call.
Accuracy: the render-level sums of both modes against the float64 render backward over fuzz cases (tests/test_gpu_fuzz.py::_case), in
units of the reference build's error on the same case -- the table of profiles/r06_bwd_accuracy.txt (max over elements of |error| /
max|g|, geomean over the cases of library / reference build).
--resources FILE: the compiler's -Rpass-analysis=kernel-resource-usage remarks of render_bwd.hip, appended as a table; without it the
script compiles the file itself."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-pcloud-render_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def resource_remarks():
    """hipcc's kernel-resource-usage remarks for render_bwd.hip, device side only, with the library's flags"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gsr_build", os.path.join(ROOT, "gaussian-pcloud-render_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    r = subprocess.run([b.HIPCC] + b.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                              os.path.join(b.CSRC, "render_bwd.hip"), "-o", os.devnull], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return r.stderr


def resource_table(text):
    """one line per colour backward kernel: VGPRs, SGPRs, scratch bytes per lane, LDS bytes per workgroup, waves per SIMD"""
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = dict(sym=m.group(1))
            rows.append(cur)
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    by = {}
    for r in rows:
        m = re.search(r"k_render_backwardILi(\d)ELi0EJ", r["sym"])
        if m and "RenderBwdX" not in r["sym"]:
            by[(int(m.group(1)), "RenderBwdDet" in r["sym"], "RenderBwdFast" in r["sym"])] = r
    out = ["%-34s %-6s %6s %6s %8s %8s %10s" % ("kernel", "mode", "VGPRs", "SGPRs", "scratch", "LDS B", "waves/SIMD")]
    bad = []
    for det in (False, True):
        for mode in (0, 1, 2):
            for fast in (False, True):
                r = by[(mode, det, fast)]
                out.append("%-34s %-6s %6d %6d %8d %8d %10d" % ("k_render_backward<%d, 0%s>" % (mode, ", Det" if det else ""),
                                                               "fast" if fast else "exact", r["vgpr"], r["sgpr"], r["scratch"], r["lds"], r["occ"]))
            if by[(mode, det, True)]["scratch"] > by[(mode, det, False)]["scratch"] or by[(mode, det, True)]["occ"] < by[(mode, det, False)]["occ"]:
                bad.append("<%d%s>" % (mode, ", Det" if det else ""))
    out.append("fast variants: " + ("no more scratch and no fewer waves per SIMD than their exact twins" if not bad
                                    else "more scratch or fewer waves than the exact twin: " + ", ".join(bad)))
    return out, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cases", type=int, default=96)
    ap.add_argument("--points", type=int, default=800_000)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def resources():
        say("registers, LDS, scratch and occupancy of the colour backward kernels from the compile (-Rpass-analysis=kernel-resource-usage, gfx950):")
        table, bad = resource_table(open(a.resources).read() if a.resources else resource_remarks())
        for row in table:
            say("   " + row)
        return bad

    if a.resources_only:
        resources()
        finish()
        return 0

    import numpy as np
    import torch
    from diff_gaussian_rasterization import _native as N
    import native_calls as NC
    dev = torch.device("cuda:0")

    def spread(xs):
        return statistics.median(xs), min(xs), max(xs)

    def report(what, d):
        (m0, lo0, hi0), (m1, lo1, hi1) = spread(d[0]), spread(d[1])
        say("   %-28s exact %8.4f ms (blocks %8.4f .. %8.4f)   fast %8.4f ms (blocks %8.4f .. %8.4f)   fast / exact %.3f   %s"
            % (what, m0, lo0, hi0, m1, lo1, hi1, m1 / m0,
               "outside the spread between blocks" if (hi1 < lo0 or lo1 > hi0) else "INSIDE the spread between blocks"))

    was = N.lib.gsr_set_train_math(-1)
    try:
        say("exact (gsr_set_train_math(0)) against fast (1), alternating blocks of %d forward + backward calls, median of %d blocks per mode; %s"
            % (a.calls, a.blocks, N.lib.gsr_version().decode()))
        W, H = 1920, 1080
        for V in (12, 1):
            g, views, _, _ = NC.circle_scene(V, P=a.points, W=W, H=H)
            args = NC.cloud_args(g, views, W, H, dev, (1.0, 1.0, 1.0))
            dpix = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (V, 3, H, W)).astype(np.float32)).to(dev)
            N.rasterize_gaussians_batch(*args, need_backward=True)      # (the next call's arena is sized from this one's counts)
            pairs = None

            def call(det):
                run = N.rasterize_gaussians_batch(*args, need_backward=True)
                counts, color, radii, geom, binning, img = run
                N.rasterize_gaussians_backward_batch(args[0], args[1], radii, args[2], args[4], args[5], args[6], args[7], args[8], args[9],
                                                     args[10], args[11], dpix, args[14], args[15], args[16], geom, binning, img, False,
                                                     deterministic=det, pairs=pairs if det else None)
                return color
            say("headline cloud (%d points, %d x %d), forward + backward, %d view%s per call; ms per CALL" % (a.points, W, H, V, "s" if V > 1 else ""))
            frames = {}
            for det in (False, True):
                if det:
                    pairs = N.last_list_pairs(V)
                for mode in (0, 1):
                    N.lib.gsr_set_train_math(mode)
                    for _ in range(3):
                        call(det)
                torch.cuda.synchronize()
                fwd, bwd, whole = {0: [], 1: []}, {0: [], 1: []}, {0: [], 1: []}
                for _ in range(a.blocks):
                    for mode in (0, 1):
                        N.lib.gsr_set_train_math(mode)
                        N.set_profiling(2)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.calls):
                            frames[mode] = call(det)
                        e1.record()
                        torch.cuda.synchronize()
                        prof = N.get_profile()
                        N.set_profiling(0)
                        fwd[mode].append(sum(ms for n, ms in prof if n == "render_forward") / a.calls)
                        bwd[mode].append(sum(ms for n, ms in prof if n == "render_backward") / a.calls)
                        whole[mode].append(e0.elapsed_time(e1) / a.calls)
                flush = "storing flush" if det else "atomic flush"
                if not det:
                    report("forward render kernel", fwd)
                report("backward render, %s" % flush, bwd)
                report("whole call, %s" % flush, whole)
            err = (frames[0].double() - frames[1].double()).abs().amax(dim=1 if V > 1 else 0)
            say("   pixels over 1e-4 between the modes' images: %d of %d (largest difference %.3g)" % (int((err > 1e-4).sum()), err.numel(), float(err.max())))
            del args, dpix, frames
            torch.cuda.empty_cache()

        # ---- accuracy of the render-level sums against float64, in units of the reference build's error
        import util
        import sweep_support as FZ
        from oracle.oracle import Oracle, Reference
        import scripts.bwd_accuracy as BA
        ref, orc = Reference("strict"), Oracle()
        names = ("mean2D", "conic", "colour", "opacity")
        sl = dict(mean2D=slice(0, 2), conic=slice(2, 5), colour=slice(5, 8), opacity=slice(8, 9))
        ratio = {m: {n: [] for n in names} for m in (0, 1)}
        used = 0
        for c in range(a.cases):
            s, _ = FZ.random_case(c)
            if s.P == 0:
                continue
            dL = util.seeded_dL(s, seed=77 + c)
            _, gr = ref.forward_backward(s, dL)
            _, go = orc.forward_backward(s, dL, exact=True)
            go = go["exact"]
            want = dict(mean2D=np.asarray(go["dL_dmean2D"], np.float64).reshape(s.P, -1)[:, :2],
                        conic=np.asarray(go["dL_dconic"], np.float64).reshape(s.P, 4)[:, [0, 1, 3]],
                        colour=np.asarray(go["dL_dcolor"], np.float64).reshape(s.P, 3),
                        opacity=np.asarray(go["dL_dopacity"], np.float64).reshape(s.P, 1))
            build = dict(mean2D=np.asarray(gr["dL_dmean2D"], np.float64).reshape(s.P, -1)[:, :2],
                         conic=np.asarray(gr["dL_dconic"], np.float64).reshape(s.P, 4)[:, [0, 1, 3]],
                         colour=np.asarray(gr["dL_dcolor"], np.float64).reshape(s.P, 3),
                         opacity=np.asarray(gr["dL_dopacity"], np.float64).reshape(s.P, 1))
            if any(np.abs(want[n]).max() == 0 for n in names):
                continue
            used += 1
            for mode in (0, 1):
                N.lib.gsr_set_train_math(mode)
                rec = BA.grad_records(s, dev, dL)
                for n in names:
                    m = np.abs(want[n]).max()
                    el, eb = np.abs(rec[:, sl[n]] - want[n]).max() / m, np.abs(build[n] - want[n]).max() / m
                    ratio[mode][n].append((el + 1e-30) / (eb + 1e-30))
        say()
        say("render-level sums against the float64 render backward, %d fuzz cases with visible splats (of %d), moments mode %d: error = max over "
            "elements in units of max|g|;" % (used, a.cases, N.lib.gsr_set_backward_moments(-1)))
        say("geomean over the cases of library / reference build (a case where the fast forward decides differently from float64 counts like any other):")
        say("   %-8s %8s %8s %8s %8s" % (("mode",) + names))
        for mode in (0, 1):
            say("   %-8s %s" % ("fast" if mode else "exact", " ".join("%7.2fx" % float(np.exp(np.mean(np.log(ratio[mode][n])))) for n in names)))
        say("   median:")
        for mode in (0, 1):
            say("   %-8s %s" % ("fast" if mode else "exact", " ".join("%7.2fx" % float(np.median(ratio[mode][n])) for n in names)))
    finally:
        N.lib.gsr_set_train_math(was)
        N.set_profiling(0)
    say()
    resources()
    finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
