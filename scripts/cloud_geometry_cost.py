"""What the point-cloud neighbourhood entries (gsr_knn, gsr_cloud_geometry) cost next to a torch formulation of the same results on the same
GPU, in ONE process, the variants alternating.

    python scripts/cloud_geometry_cost.py [--rounds 10] [--warmup 2] [--torch-rounds 2] [--torch-budget 40] [--out profiles/r26_cloud_geometry.txt]

Workloads: synth-THuman-800K (800 000 float points on the capsule body) and synth-THuman-256 (200 000 voxelised points: a lattice, every
distance tied many times over).  Variants per cloud: gsr_knn with K = 3 and K = 16 (scratch allocated outside the timed window, as a
caller that keeps it would), gsr_cloud_geometry with all five outputs on the K = 16 lists, and the torch formulation: chunked
torch.cdist + topk(K + 1, largest=False) minus the point itself for the lists, and for the geometry a gather of the neighbours, their
covariance by batched matmul and torch.linalg.eigh.  The torch k-NN is seconds per round at 800 K: it is first timed on 32 chunks, and
run in full (--torch-rounds rounds) only when that predicts a round within --torch-budget seconds; otherwise the figure is the 32-chunk
time scaled by the number of chunks (cdist and topk are linear in the number of queries) and the table says so.

Reported: median (min .. max) ms between two device events, and the multiple of a byte model at the bandwidth benchlib.roofline takes
as achievable.  gsr_knn per point: 12 B read by the box reduction, 12 + 4 by the keys, 76 by the four sort passes (4 B counted, 8 + 8
scattered; the first pass reads no values), 4 + 12 + 16 by the gather, 16 read once by the search and 8 K written: 152 + 8 K.
gsr_cloud_geometry per point: 12 + 4 K read, 12 K gathered, 68 written.  The search is arithmetic, not traffic: its multiple of the
byte model says how far from a copy it is, nothing more.  The times are written down as they come out: no bar is set on them."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-pcloud-render_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

CHUNK = 1024
PROBE_CHUNKS = 32


def torch_knn_chunks(pts, K, first, count):
    """the lists of queries [first * CHUNK, (first + count) * CHUNK) against the whole cloud: (idx, d2)"""
    import torch
    out_i, out_d = [], []
    for c in range(first, first + count):
        q = pts[c * CHUNK:(c + 1) * CHUNK]
        if q.shape[0] == 0:
            break
        d = torch.cdist(q, pts)
        d[torch.arange(q.shape[0], device=pts.device), torch.arange(c * CHUNK, c * CHUNK + q.shape[0], device=pts.device)] = float("inf")
        v, i = torch.topk(d, K, dim=1, largest=False)
        out_i.append(i)
        out_d.append(v * v)
    return torch.cat(out_i), torch.cat(out_d)


def torch_geometry(pts, idx, k_s=3):
    """spacing, covariance, eigenvalues and normals of full lists (no padding) in torch"""
    import torch
    nb = pts[idx.long()] - pts[:, None, :]                                  # [P, K, 3]
    spacing = (nb[:, :k_s] ** 2).sum(-1).mean(1).sqrt()
    hood = torch.cat([torch.zeros_like(nb[:, :1]), nb], 1)
    e = hood - hood.mean(1, keepdim=True)
    cov = e.transpose(1, 2) @ e / hood.shape[1]
    lam, vec = torch.linalg.eigh(cov)
    return spacing, cov, lam, vec[:, :, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-rounds", type=int, default=2)
    ap.add_argument("--torch-budget", type=float, default=40.0, help="seconds a full torch k-NN round may be predicted to take")
    ap.add_argument("--clouds", default="synth-THuman-800K,synth-THuman-256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from benchlib import roofline
    from diff_gaussian_rasterization import _native as N
    from pcrender import synth
    if not torch.cuda.is_available():
        raise SystemExit("cloud_geometry_cost.py measures on the GPU: no HIP device is visible")
    dev = torch.device("cuda:0")
    bw = roofline.HBM_ACHIEVABLE_GBS * 1e9
    say("point-cloud neighbourhoods in HIP against a torch formulation; %s" % N.lib.gsr_version().decode())

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    for name in a.clouds.split(","):
        cloud = synth.make_cloud(name, seed=0)
        pts = torch.from_numpy(np.ascontiguousarray(cloud["means3D"])).to(dev)
        P = pts.shape[0]
        nchunks = -(-P // CHUNK)
        say()
        say("%s: P = %d points" % (name, P))
        stream = torch.cuda.current_stream(dev).cuda_stream
        bufs = {}
        for K in (3, 16):
            nbytes = N.lib.gsr_knn_scratch_bytes(P, K)
            bufs[K] = (torch.empty((P, K), dtype=torch.int32, device=dev), torch.empty((P, K), dtype=torch.float32, device=dev),
                       torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes)

        def run_knn(K):
            idx, d2, scratch, nbytes = bufs[K]
            rc = N.lib.gsr_knn(P, pts.data_ptr(), K, idx.data_ptr(), d2.data_ptr(), scratch.data_ptr(), nbytes, stream)
            if rc != 0:
                raise RuntimeError(N.lib.gsr_last_error().decode())

        geo = {w: torch.empty((P,) + N._CLOUD_WIDTH[w], dtype=torch.float32, device=dev) for w in N.CLOUD_OUTPUTS}

        def run_geometry():
            rc = N.lib.gsr_cloud_geometry(P, pts.data_ptr(), 16, bufs[16][0].data_ptr(), 3, 16, None, *[geo[w].data_ptr() for w in N.CLOUD_OUTPUTS],
                                          stream)
            if rc != 0:
                raise RuntimeError(N.lib.gsr_last_error().decode())

        state = {}

        def run_torch_geometry():
            state["tg"] = torch_geometry(pts, bufs[16][0])

        variants = [("gsr_knn K = 3", lambda: run_knn(3)), ("gsr_knn K = 16", lambda: run_knn(16)), ("gsr_cloud_geometry K = 16", run_geometry),
                    ("torch gather + matmul + linalg.eigh, K = 16", run_torch_geometry)]
        ms = {k: [] for k, _ in variants}
        run_knn(16)                                                            # the geometry variants read these lists
        for r in range(a.warmup + a.rounds):
            for vname, fn in variants:
                t, _ = timed(fn)
                if r >= a.warmup:
                    ms[vname].append(t)
        model = {"gsr_knn K = 3": (152 + 8 * 3) * P / bw * 1e3, "gsr_knn K = 16": (152 + 8 * 16) * P / bw * 1e3,
                 "gsr_cloud_geometry K = 16": (12 + 16 * 16 + 68) * P / bw * 1e3}
        model["torch gather + matmul + linalg.eigh, K = 16"] = model["gsr_cloud_geometry K = 16"]
        say("  ms, median (min .. max) of %d alternating rounds after %d warm-up rounds; byte model at %.0f GB/s" % (a.rounds, a.warmup, bw / 1e9))
        say("  %-46s %26s %9s %9s" % ("variant", "ms", "model ms", "x model"))
        for vname, _ in variants:
            m = statistics.median(ms[vname])
            say("  %-46s %9.3f (%.3f .. %.3f) %9.4f %9.1f" % (vname, m, min(ms[vname]), max(ms[vname]), model[vname], m / model[vname]))
        g_hip, g_torch = statistics.median(ms["gsr_cloud_geometry K = 16"]), statistics.median(ms["torch gather + matmul + linalg.eigh, K = 16"])
        say("  geometry: HIP %.3f ms, torch %.3f ms: %.1f x" % (g_hip, g_torch, g_torch / g_hip))

        # the torch k-NN: a probe of PROBE_CHUNKS chunks first, a full round only within the budget
        for K in (3, 16):
            probe = min(PROBE_CHUNKS, nchunks)
            timed(lambda: torch_knn_chunks(pts, K, 0, 2))                      # warm-up
            t_probe, _ = timed(lambda: torch_knn_chunks(pts, K, 0, probe))
            predicted = t_probe * nchunks / probe
            hip = statistics.median(ms["gsr_knn K = %d" % K])
            if predicted / 1e3 <= a.torch_budget:
                full = []
                for _ in range(a.torch_rounds):
                    t0 = time.time()
                    t, (ti, td) = timed(lambda: torch_knn_chunks(pts, K, 0, nchunks))
                    full.append(t)
                    if time.time() - t0 > a.torch_budget:
                        break
                tm = statistics.median(full)
                say("  torch cdist + topk, K = %-2d  %10.1f ms (median of %d full rounds, chunks of %d queries; the %d-chunk probe predicted %.1f): %.0f x gsr_knn"
                    % (K, tm, len(full), CHUNK, probe, predicted, tm / hip))
                # faster and different is not faster: the same neighbours wherever distances are not tied
                hi, hd = bufs[K][0], bufs[K][1]
                same_d = float((hd.sqrt() - td.sqrt()).abs().max())
                same_i = float((hi.long() == ti).float().mean())
                say("    agreement: largest difference of the distances %.3g, %.2f %% of the indices identical (ties and cdist's rounding order the rest differently)"
                    % (same_d, 100 * same_i))
                del ti, td
            else:
                say("  torch cdist + topk, K = %-2d  %10.1f ms SCALED from %d of %d chunks (%.1f ms measured; a full round is beyond the %.0f s budget): %.0f x gsr_knn"
                    % (K, predicted, probe, nchunks, t_probe, a.torch_budget, predicted / hip))
            torch.cuda.empty_cache()
        del bufs, geo, state
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f_:
            f_.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
