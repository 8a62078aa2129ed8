"""What the fast arithmetic of the inference forwards (gsr_set_render_math(1), csrc/render_math.hpp) costs and buys against the exact
mode of the same build, in ONE process: exact and fast blocks ALTERNATE after a warm-up, every figure is the median over the blocks
and the spread between blocks is printed next to it (a difference inside the spread is no difference).

    python scripts/render_math_cost.py [--blocks 7] [--calls 5] [--resources FILE] [--out profiles/r12_render_math.txt]
    python scripts/render_math_cost.py --resources-only          (no GPU: compiles render_fwd.hip for the device and prints the table)

Workloads:
  * the headline cloud (synth-THuman-800K, training profile, 1920 x 1080), forward only: 12 views per call (k_render_forward<0>) and
    1 view per call (k_render_forward_half);
  * render_passes, 12 views x 4 passes at 512^2 x super-sample 2 on the 200 K cloud: without normals (nx = 4) and with (nx = 8).
Per workload and mode: the render kernel (gsr_set_profiling(2): one event pair around it) and the whole call (device events around the
block of calls), ms per call; and the share of pixels of those frames whose largest channel difference between the modes exceeds 1e-4.
--resources FILE: the compiler's -Rpass-analysis=kernel-resource-usage remarks of render_fwd.hip (registers, LDS, scratch, occupancy
of the exact and the fast instantiations), appended as a table; without it the script compiles the file itself."""
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
    """hipcc's kernel-resource-usage remarks for render_fwd.hip, device side only, with the library's flags"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gsr_build", os.path.join(ROOT, "gaussian-pcloud-render_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    r = subprocess.run([b.HIPCC] + b.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                              os.path.join(b.CSRC, "render_fwd.hip"), "-o", os.devnull], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return r.stderr


def resource_table(text):
    """one line per forward kernel: VGPRs, SGPRs, scratch bytes per lane, LDS bytes per workgroup, waves per SIMD"""
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

    def name(sym):
        fast = "RenderFast" in sym
        m = re.search(r"k_render_forwardILi(\d)E", sym)
        base = "k_render_forward<%s>" % m.group(1) if m else "k_render_forward_half"
        return base, fast
    out = ["%-24s %-6s %6s %6s %8s %8s %10s" % ("kernel", "mode", "VGPRs", "SGPRs", "scratch", "LDS B", "waves/SIMD")]
    by = {}
    for r in rows:
        if "k_render_forward" not in r["sym"]:
            continue
        base, fast = name(r["sym"])
        by[(base, fast)] = r
    bad = []
    for base in ("k_render_forward<0>", "k_render_forward_half", "k_render_forward<4>", "k_render_forward<8>"):
        for fast in (False, True):
            r = by[(base, fast)]
            out.append("%-24s %-6s %6d %6d %8d %8d %10d" % (base, "fast" if fast else "exact", r["vgpr"], r["sgpr"], r["scratch"], r["lds"], r["occ"]))
        if by[(base, True)]["scratch"] != 0 or by[(base, True)]["occ"] < by[(base, False)]["occ"]:
            bad.append(base)
    out.append("fast variants: " + ("no scratch, no fewer waves per SIMD than their exact twins" if not bad else "WORSE than exact: " + ", ".join(bad)))
    return out, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
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
        say("registers, LDS, scratch and occupancy from the compile (-Rpass-analysis=kernel-resource-usage, gfx950):")
        table, bad = resource_table(open(a.resources).read() if a.resources else resource_remarks())
        for row in table:
            say("   " + row)
        return bad

    if a.resources_only:
        bad = resources()
        finish()
        return 1 if bad else 0

    import numpy as np
    import torch
    from diff_gaussian_rasterization import _native as N
    from pcrender import camera, raster_passes as rp, synth
    dev = torch.device("cuda:0")

    def t(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def median_spread(xs):
        return statistics.median(xs), min(xs), max(xs)

    def measure(title, call, frames):
        """call() makes one inference call; frames(its result) gives {name: (image tensor, its channel axis)}"""
        for mode in (0, 1):
            N.lib.gsr_set_render_math(mode)
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        kern, whole = {0: [], 1: []}, {0: [], 1: []}
        for _ in range(a.blocks):
            for mode in (0, 1):
                N.lib.gsr_set_render_math(mode)
                N.set_profiling(2)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                prof = [ms for name, ms in N.get_profile() if name == "render_forward"]
                N.set_profiling(0)
                kern[mode].append(sum(prof) / a.calls)
                whole[mode].append(e0.elapsed_time(e1) / a.calls)
        say(title)
        for what, d in (("render kernel", kern), ("whole call", whole)):
            (m0, lo0, hi0), (m1, lo1, hi1) = median_spread(d[0]), median_spread(d[1])
            say("   %-14s exact %8.4f ms (blocks %8.4f .. %8.4f)   fast %8.4f ms (blocks %8.4f .. %8.4f)   fast / exact %.3f   %s"
                % (what, m0, lo0, hi0, m1, lo1, hi1, m1 / m0,
                   "outside the spread between blocks" if (hi1 < lo0 or lo1 > hi0) else "INSIDE the spread between blocks"))
        N.lib.gsr_set_render_math(0)
        fe = frames(call())
        N.lib.gsr_set_render_math(1)
        ff = frames(call())
        for k in fe:
            x, chan_dim = fe[k]
            y, _ = ff[k]
            err = (x.double() - y.double()).abs().amax(dim=chan_dim)
            say("   %-14s pixels over 1e-4 between the modes: %d of %d (share %.3g), largest difference %.3g, median %.3g"
                % (k, int((err > 1e-4).sum()), err.numel(), float((err > 1e-4).double().mean()), float(err.max()), float(err.median())))
        torch.cuda.synchronize()

    was = N.lib.gsr_set_render_math(-1)
    try:
        say("exact (gsr_set_render_math(0)) against fast (1), alternating blocks of %d calls, median of %d blocks per mode; %s"
            % (a.calls, a.blocks, N.lib.gsr_version().decode()))
        # ---- the headline cloud, forward only
        W, H = 1920, 1080
        cloud = synth.make_cloud("synth-THuman-800K", seed=0)
        g = synth.make_gaussians(cloud, profile="training", seed=1)
        views = camera.circle_views(12, fov_deg=45.0, width_px=W, height_px=H)
        e = torch.empty(0)
        vm = torch.stack([v["viewmatrix"] for v in views]).to(dev)
        pm = torch.stack([v["projmatrix"] for v in views]).to(dev)
        cp = torch.stack([v["campos"] for v in views]).to(dev)
        args = [t(np.ones(3, np.float32)), t(g["means3D"]), e, t(g["opacities"]), t(g["scales"]), t(g["rotations"]), 1.0, e, vm, pm,
                views[0]["tanfovx"], views[0]["tanfovy"], H, W, t(g["shs"]), g["sh_degree"], cp, False, False]
        with torch.no_grad():
            measure("headline cloud (%d points, %d x %d), forward only, 12 views per call [k_render_forward<0>]; ms per CALL of 12 views"
                    % (g["means3D"].shape[0], W, H),
                    lambda: N.rasterize_gaussians_batch(*args, need_backward=False), lambda r: {"rgb": (r[1], 1)})
            one = list(args)
            one[8], one[9], one[16] = vm[0], pm[0], cp[0]
            measure("headline cloud, forward only, 1 view per call [k_render_forward_half]",
                    lambda: N.rasterize_gaussians(*one, need_backward=False), lambda r: {"rgb": (r[1], 0)})
        del args, one, g, cloud
        torch.cuda.empty_cache()
        # ---- render_passes on the 200 K cloud
        cloud = synth.make_cloud("synth-THuman-256", seed=0)
        g = synth.make_gaussians(cloud, profile="inference", seed=1)
        sf = cloud["scale_factor"]
        radius = float(np.sqrt(3) / sf * 6)
        means, shs, opac, rots = t(g["means3D"]), t(g["shs"]), t(g["opacities"]), t(g["rotations"])
        dec_s = t((g["scales"] / radius).astype(np.float32))
        normals = torch.nn.functional.normalize(means, dim=-1)
        Hs = camera.circle_path(12, 0, 3, [90, 0])
        bg = torch.ones(3)
        for nx, nrm in ((4, None), (8, normals)):
            measure("render_passes, 12 views x 4 passes, 512^2 x super-sample 2, %d points, nx = %d [k_render_forward<%d>]; frames after the down-filter"
                    % (means.shape[0], nx, nx),
                    lambda: rp.render_passes(means, opac, dec_s, rots, shs, Hs, 512, 512, 45.0, bg, sf, normals=nrm),
                    lambda r: {k: (v, -1) for k, v in r.items() if v is not None})
    finally:
        N.lib.gsr_set_render_math(was)
        N.set_profiling(0)
    say()
    resources()
    finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
