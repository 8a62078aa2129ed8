"""Seeded cases of the EXTRA-CHANNEL calls (gsr_forward_batch_channels, gsr_forward_batch_channels_train, gsr_backward_batch_channels)
for the channels sweep, on top of tests/batch_cases.py: a case is one of that generator's view batches (cloud, views, image, options;
nothing of it is restated here) plus seeded channel draws.  Importable without a GPU.

  case(i)      batch_cases.case(SMALL_FROM[i]) (small, i = 0 .. n-1) or batch_cases' medium case MEDIUM_FROM[i - MEDIUM_BASE], with
               nx in {4, 8}, the layout of the values (0 shared [P,nx], 1 per view [V,P,nx], 2 split ([P,4], [V,P,4]); 2 only with
               nx = 8), view scales [V,nx] or None, bg_extra [nx], the values in the layout's shape and the dense [V,P,nx] values
               they stand for, dL_dpix [V,3,H,W] and dL_dextra [V,nx,H,W] (test_gpu_channels_fp64._inputs draws them)
  expected(i)  batch_cases.expected of the batch plus the channel draws: what the census of tests/test_cpu_channel_cases.py counts
  fingerprint  a hash of every byte of a case

The view scales come in two classes.  "exact" (three quarters of the cases): {-2, -1, -0.5, 0, 0.5, 1, 2}, powers of two, so that
value x scale x alpha x T is the same float32 number in whatever order the factors are multiplied.  "rounded" (i % 4 == 3, and the
second medium case): {-1.7, 3.0, 0.3}, where float32(value x scale) x alpha differs from value x (scale x alpha).

The first six cases are batch_cases' pinned ones (256 views; 64 views of 704 tiles; the three slabs of mixed depth-sort pass counts;
empty views 0 / 6 / 12).  Only the batch cases 0 and 1 make k_render_backward pull its work units (ceil(T / 8) V > 4096 needs 47
views of the largest image), and each of the three layouts has to meet that launch: batch case 1 is therefore listed twice, with
different channel draws."""
import hashlib

import numpy as np

import batch_cases as BC

F = np.float32
N_SMALL = 48
MEDIUM_BASE = BC.MEDIUM_BASE
# indices into batch_cases' small class (batch case 40 is left out on purpose: one of its splats is so ill-conditioned that two atomic
# backwards of the same arenas differ by more than the element bar of util.check_grads, tests/test_gpu_channel_fuzz.py)
SMALL_FROM = [0, 1, 2, 3, 4, 5, 1, 7, 8, 10, 11, 12, 13, 15, 17, 18, 21, 23, 24, 26, 27, 29, 30, 32, 33, 35, 36, 37, 52, 44, 49, 53,
              54, 55, 56, 58, 62, 64, 67, 68, 69, 73, 76, 77, 85, 86, 88, 91]
# indices into batch_cases.MEDIUM: (5, 300000, 64, 48) a ragged last row, (13, 150000, 272, 256) more than 255 tiles,
# (17, 70000, 112, 96) vpt 2 rows 8x2+1
MEDIUM_FROM = [0, 5, 6]
# the first medium case keeps the first 262 144 of its 300 000 points: the fewest that still give k_preprocess 4 views per thread in
# 2 grid rows (1024 blocks), since its float64 reference -- three oracle runs per view here, one in the colour sweep -- is most of
# the case's time
MEDIUM_POINTS = {0: 262144}
EXACT_SCALES = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], F)
ROUNDED_SCALES = np.array([-1.7, 3.0, 0.3], F)
# channel draws fixed so that the census holds whatever the seeds give (like batch_cases.PINNED): every layout under the pulled
# backward units (0, 1, 6), the split layout on slabs of mixed pass counts (2; 42: two views) and on empty views (5), a call without
# view scales (4); the rounded scales of the second medium case present, and the medium cases on three different layouts
PINNED = {0: dict(nx=8, layout=2), 1: dict(nx=8, layout=1), 6: dict(nx=4, layout=0), 2: dict(nx=8, layout=2), 3: dict(nx=4, layout=1),
          4: dict(nx=8, layout=0, no_scale=True), 5: dict(nx=8, layout=2), 42: dict(nx=8, layout=2),
          MEDIUM_BASE: dict(nx=4, layout=0, no_scale=False), MEDIUM_BASE + 1: dict(nx=8, layout=2, no_scale=False),
          MEDIUM_BASE + 2: dict(nx=8, layout=1, no_scale=False)}

assert len(SMALL_FROM) == N_SMALL and SMALL_FROM[:6] == [0, 1, 2, 3, 4, 5]


def ids(n_small=N_SMALL):
    return list(range(min(n_small, N_SMALL))) + [MEDIUM_BASE + j for j in range(len(MEDIUM_FROM))]


def batch_index(i):
    return BC.MEDIUM_BASE + MEDIUM_FROM[i - MEDIUM_BASE] if i >= MEDIUM_BASE else SMALL_FROM[i]


def draws(i):
    """the channel draws that do not need the batch: dict(nx, layout, no_scale, scale_class)"""
    rng = np.random.default_rng(12000 + i)
    nx = int(rng.choice([4, 8]))
    layout = int(rng.choice([0, 1] if nx == 4 else [0, 1, 2]))
    no_scale = bool(rng.random() < 0.12)
    pin = PINNED.get(i, {})
    rounded = (i - MEDIUM_BASE == 1) if i >= MEDIUM_BASE else (i % 4 == 3)
    return dict(nx=pin.get("nx", nx), layout=pin.get("layout", layout), no_scale=pin.get("no_scale", no_scale),
                scale_class="rounded" if rounded else "exact")


def case(i):
    from fp64_pins import channel_inputs
    c = BC.case(batch_index(i))
    d = draws(i)
    if i >= MEDIUM_BASE and i - MEDIUM_BASE in MEDIUM_POINTS:
        P0, P1 = c["g"]["means3D"].shape[0], MEDIUM_POINTS[i - MEDIUM_BASE]
        c["g"] = {k: a[:P1] if isinstance(a, np.ndarray) and a.shape[0] == P0 else a for k, a in c["g"].items()}
    V, P = len(c["views"]), c["g"]["means3D"].shape[0]
    x, dense, sc, bgx, dpix, dx = channel_inputs(P, V, d["nx"], d["layout"], seed=13000 + i, H=c["H"], W=c["W"],
                                          scales=ROUNDED_SCALES if d["scale_class"] == "rounded" else EXACT_SCALES)
    return dict(d, i=i, batch=c, x=x, dense=dense, scale=None if d["no_scale"] else sc, bg_extra=bgx, dpix=dpix, dx=dx)


def expected(i, c=None):
    """batch_cases.expected of the case's batch, and its channel draws"""
    e = dict(BC.expected(batch_index(i), None if c is None else c["batch"]))
    e.update(draws(i))
    return e


def fingerprint(c):
    h = hashlib.sha256()
    h.update(BC.fingerprint(c["batch"]).encode())
    h.update(repr((c["nx"], c["layout"], c["no_scale"], c["scale_class"])).encode())
    for a in (c["x"] if isinstance(c["x"], tuple) else (c["x"],)) + (c["dense"], c["bg_extra"], c["dpix"], c["dx"]):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(b"none" if c["scale"] is None else np.ascontiguousarray(c["scale"]).tobytes())
    return h.hexdigest()
