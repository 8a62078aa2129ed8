"""Host references of the point-cloud neighbourhood entries (include/gsr.h gsr_knn, gsr_cloud_geometry) and the cases their tests share.

  knn_brute      the definition by brute force in numpy float32: d2 with the header's written operations, the K smallest (d2, j) per row
                 through one 64-bit key (the float32 bits of d2, which order like the non-negative numbers they stand for, above the
                 index), chunked partition + sort.
  geometry       spacing, covariance, Jacobi, normal and quaternion op by op in the header's order, in the dtype asked for: float32 is the
                 restatement the device has to match bit for bit, float64 the same algorithm without its rounding.
  eigh64         numpy.linalg.eigh in float64 on a float32 cov6: what the Jacobi iteration is held to.
  CASES          the clouds, KS the list lengths.
The constants come from the sources (include/gsr.h, csrc/cloud_geometry.hpp)."""
import collections
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "gsr.h")).read()
_HPP = open(os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc", "cloud_geometry.hpp")).read() \
    if os.path.exists(os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc", "cloud_geometry.hpp")) else ""


def _const(text, name, default):
    m = re.search(r"\b%s\s*=?\s*(\d+)" % name, text)
    return int(m.group(1)) if m else default


SWEEPS = _const(_HEADER, "GSR_CLOUD_JACOBI_SWEEPS", 5)
RUN = _const(_HPP, "CLOUD_RUN", 64)
COARSE = _const(_HPP, "CLOUD_COARSE", 64)
MAX_K = _const(_HPP, "CLOUD_MAX_K", 32)
KS = (1, 3, 16, 32)
F32 = np.float32

# The bars of the float32 Jacobi iteration against numpy.linalg.eigh in float64 on the same float32 cov6, relative to the largest
# eigenvalue: 4 x the worst error measured on the CPU over every case of CASES with SWEEPS sweeps (tests/test_cpu_cloud_ref.py prints and
# asserts worst / bar).  Worst measured: eigenvalues 2.51e-7, reconstruction 7.63e-7, the same figures with 4, 5, 6, 7 and 8 sweeps: the
# iteration has converged after 4 and what is left is the rounding of its rotations.  SWEEPS = 5 is one sweep past that.
EIGENVALUE_BAR = 1.0e-6
RECONSTRUCTION_BAR = 3.1e-6
# The normal of a surface case against the analytic one, in degrees: the float64 reference's p99 is under 7 on every surface case.
NORMAL_P99_BAR_DEG = 7.0
# A normal is compared with the float64 eigenvector only where the two smallest eigenvalues are apart: (l1 - l0) / l2 >= GAP_RULE
GAP_RULE = 0.05
GAP_RULE_MAX_LEFT_OUT = 0.01
# ... and there within the perturbation bound of a symmetric eigenvector: |E| / gap with |E| <= RECONSTRUCTION_BAR l2 and gap >=
# GAP_RULE l2, in degrees (0.0036; measured 1.3e-5)
EIGENVECTOR_BAR_DEG = float(np.degrees(RECONSTRUCTION_BAR / GAP_RULE))

Case = collections.namedtuple("Case", "name P kind seed")


def _rng(c):
    return np.random.default_rng(1000 + c.seed)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def surface(kind, P, rng, noise):
    """(points float32 [P,3], analytic unit normals float64 [P,3]) of a noisy sphere, plane or torus"""
    if kind == "sphere":
        n = _unit(rng.standard_normal((P, 3)))
        p = n.copy()
    elif kind == "plane":
        p = np.concatenate([rng.uniform(-1, 1, (P, 2)), np.zeros((P, 1))], 1)
        n = np.tile(np.array([[0.3, -0.2, 1.0]]), (P, 1))
        n = _unit(n)
        # the plane through the origin with that normal: lift z so that p . n = 0
        p[:, 2] = -(p[:, 0] * n[0, 0] + p[:, 1] * n[0, 1]) / n[0, 2]
    else:
        u, v = rng.uniform(0, 2 * np.pi, P), rng.uniform(0, 2 * np.pi, P)
        ring = np.stack([np.cos(u), np.sin(u), np.zeros(P)], 1)
        n = ring * np.cos(v)[:, None] + np.array([[0, 0, 1.0]]) * np.sin(v)[:, None]
        p = ring * 1.0 + 0.4 * n
    p = p + noise * rng.standard_normal((P, 3))
    return p.astype(F32), n


SURFACE_NOISE = {4097: 0.002, 8193: 0.001}


def make_points(c):
    """the cloud of a case, float32 [P, 3]"""
    rng, P = _rng(c), c.P
    if c.kind in ("sphere", "plane", "torus"):
        return surface(c.kind, P, rng, SURFACE_NOISE.get(P, 0.002))[0]
    if c.kind == "lattice":                 # all ties: the project's voxelised clouds
        g = np.arange(12, dtype=F32)
        p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return p[rng.permutation(len(p))][:P].copy()
    if c.kind == "repeated":                # every point three times
        base = rng.standard_normal((P // 3, 3)).astype(F32)           # (P is a multiple of 3)
        return np.concatenate([base, base, base])[rng.permutation(3 * len(base))].copy()
    if c.kind == "identical":
        return np.tile(np.array([[0.25, -1.5, 3.0]], dtype=F32), (P, 1))
    if c.kind == "collinear":
        t = rng.uniform(-1, 1, (P, 1))
        return (t * np.array([[1.0, 2.0, -0.5]]) + np.array([[0.1, 0.2, 0.3]])).astype(F32)
    if c.kind == "outliers":                # a tight cluster and 5 points at 1e4 x its extent
        p = (0.01 * rng.standard_normal((P, 3))).astype(F32)
        p[rng.choice(P, 5, replace=False)] = (1e2 * rng.standard_normal((5, 3))).astype(F32)
        return p
    if c.kind == "offset":                  # a large common exponent
        return (1000.0 + rng.uniform(0, 1, (P, 3))).astype(F32)
    if c.kind == "nonfinite":               # 7 absent points
        p = rng.standard_normal((P, 3)).astype(F32)
        bad = rng.choice(P, 7, replace=False)
        p[bad[:3], 0] = np.nan
        p[bad[3:5], 1] = np.inf
        p[bad[5:], 2] = -np.inf
        return p
    raise ValueError(c.kind)


# the wave-run and coarse-box edges on one shape, the list lengths' own edges (P = K, K + 1), and every special cloud
EDGE_P = (1, 2, 3, 4, 16, 17, 32, 33, RUN - 1, RUN, RUN + 1, RUN * COARSE - 1, RUN * COARSE, RUN * COARSE + 1, 2 * RUN * COARSE + 1)
CASES = tuple(Case("sphere-%d" % P, P, "sphere", k) for k, P in enumerate(EDGE_P)) + (
    Case("plane-4097", 4097, "plane", 20), Case("torus-4097", 4097, "torus", 21), Case("plane-8193", 8193, "plane", 22),
    Case("torus-8193", 8193, "torus", 23), Case("lattice-1728", 1728, "lattice", 24), Case("repeated-1500", 1500, "repeated", 25),
    Case("identical-200", 200, "identical", 26), Case("collinear-700", 700, "collinear", 27), Case("outliers-4200", 4200, "outliers", 28),
    Case("offset-1000", 1000, "offset", 29), Case("nonfinite-900", 900, "nonfinite", 30), Case("nonfinite-9", 9, "nonfinite", 31))
SURFACE_CASES = tuple(c for c in CASES if c.kind in ("sphere", "plane", "torus") and c.P in SURFACE_NOISE)
_EXCLUDED = np.uint64(0xFFFFFFFFFFFFFFFF)


def present_mask(points):
    return np.isfinite(points).all(1)


def knn_brute(points, K, chunk=256, dtype=F32):
    """(idx int32 [P,K], d2 dtype [P,K]): the K present others with the smallest (d2, j) per row, ascending; -1 / +inf beyond them.
    dtype float64 (for the comparison as sets) orders by the float64 distance, ties to the lower index likewise."""
    pts = np.ascontiguousarray(points, dtype=dtype)
    P = len(pts)
    ok = present_mask(pts)
    idx = np.full((P, K), -1, np.int32)
    d2 = np.full((P, K), np.inf, dtype)
    col = np.arange(P, dtype=np.uint64)[None, :]
    shift, bits = (np.uint64(32), np.uint32) if dtype == F32 else (None, None)
    with np.errstate(all="ignore"):
        for a in range(0, P, chunk):
            q = pts[a:a + chunk]
            dx, dy, dz = (q[:, None, k] - pts[None, :, k] for k in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            out = ~ok[None, :] | ~ok[a:a + chunk, None]
            out[np.arange(len(q)), np.arange(a, a + len(q))] = True
            if dtype == F32:
                key = (d.view(bits).astype(np.uint64) << shift) | col
                key[out] = _EXCLUDED
                kk = min(K, P)
                best = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1) if kk < P else np.sort(key, axis=1)
                good = best != _EXCLUDED
                j = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
                idx[a:a + chunk, :kk] = np.where(good, j, -1)
                d2[a:a + chunk, :kk] = np.where(good, (best >> shift).astype(np.uint32).view(F32), np.inf)
            else:
                d = np.where(out, np.inf, d)
                order = np.argsort(d, axis=1, kind="stable")[:, :K]
                dd = np.take_along_axis(d, order, 1)
                kk = order.shape[1]
                idx[a:a + chunk, :kk] = np.where(np.isfinite(dd) | (np.take_along_axis(out, order, 1) == 0), order, -1)
                d2[a:a + chunk, :kk] = dd
    return idx, d2


_LISTS = {}


def case_lists(c):
    """(points, idx [P, MAX_K], d2 [P, MAX_K]) of a case, made once: a row's first K entries are its K-list"""
    if c.name not in _LISTS:
        p = make_points(c)
        _LISTS[c.name] = (p,) + knn_brute(p, MAX_K)
    return _LISTS[c.name]


def box_bound(lo, hi, q):
    """the header's float32 lower bound of d2 between q [.., 3] and any point of the box [lo, hi]"""
    lo, hi, q = (np.asarray(v, F32) for v in (lo, hi, q))
    g = np.maximum(np.maximum(lo - q, q - hi), F32(0))
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def d2_of(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _rotate(A, V, p, q, r, T):
    apq = A[p][q]
    on = apq != 0
    safe = np.where(on, apq, T(1))
    theta = (A[q][q] - A[p][p]) / (T(2) * safe)
    sgn = np.where(theta >= 0, T(1), T(-1))
    t = sgn / (np.abs(theta) + np.sqrt(theta * theta + T(1)))
    c = T(1) / np.sqrt(t * t + T(1))
    s = t * c
    h = t * apq
    new = {}
    new[(p, p)] = A[p][p] - h
    new[(q, q)] = A[q][q] + h
    new[(p, q)] = np.zeros_like(apq)
    arp, arq = A[r][p], A[r][q]
    new[(r, p)] = c * arp - s * arq
    new[(r, q)] = s * arp + c * arq
    for (i, j), v in new.items():
        A[i][j] = A[j][i] = np.where(on, v, A[i][j])
    for k in range(3):
        vkp, vkq = V[k][p], V[k][q]
        V[k][p] = np.where(on, c * vkp - s * vkq, vkp)
        V[k][q] = np.where(on, s * vkp + c * vkq, vkq)


def jacobi(cov6, sweeps=None, dtype=F32):
    """(eigenvalues [P,3] ascending, V [P,3,3] with the eigenvectors as columns) by the header's cyclic Jacobi iteration in `dtype`"""
    T = dtype
    C = np.asarray(cov6, T)
    A = [[C[:, 0], C[:, 1], C[:, 2]], [C[:, 1], C[:, 3], C[:, 4]], [C[:, 2], C[:, 4], C[:, 5]]]
    A = [[x.copy() for x in row] for row in A]
    one, zero = np.ones(len(C), T), np.zeros(len(C), T)
    V = [[one.copy() if i == j else zero.copy() for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS if sweeps is None else sweeps):
            _rotate(A, V, 0, 1, 2, T)
            _rotate(A, V, 0, 2, 1, T)
            _rotate(A, V, 1, 2, 0, T)
    lam = [A[0][0], A[1][1], A[2][2]]
    for i, j in ((0, 1), (1, 2), (0, 1)):
        sw = lam[i] > lam[j]
        lam[i], lam[j] = np.where(sw, lam[j], lam[i]), np.where(sw, lam[i], lam[j])
        for k in range(3):
            V[k][i], V[k][j] = np.where(sw, V[k][j], V[k][i]), np.where(sw, V[k][i], V[k][j])
    return np.stack(lam, 1), np.stack([np.stack(row, 1) for row in V], 1)


Geometry = collections.namedtuple("Geometry", "spacing cov6 eigenvalues normals rotations degenerate")


def geometry(points, knn_idx, k_s=3, k_n=None, orient_to=None, dtype=F32):
    """gsr_cloud_geometry op by op in `dtype` (float32: the device's bits).  knn_idx may hold any int32."""
    T = dtype
    pts = np.asarray(points, F32).astype(T)
    idx = np.asarray(knn_idx)
    P, K = idx.shape
    k_s, k_n = min(k_s, K), K if k_n is None else k_n
    finite = np.isfinite(pts).all(1)
    inside = (idx >= 0) & (idx < P)
    j = np.where(inside, idx, 0)
    pres = inside & finite[j] & finite[:, None]
    rank = np.cumsum(pres, 1) - pres                       # present entries before this one
    zero = np.zeros(P, T)
    with np.errstate(all="ignore"):
        delta = pts[j] - pts[:, None, :]                   # [P, K, 3]
        ssum, s = zero.copy(), [zero.copy() for _ in range(3)]
        for k in range(K):
            d = delta[:, k]
            use = pres[:, k] & (rank[:, k] < k_s)
            ssum = np.where(use, ssum + ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]), ssum)
            use = pres[:, k] & (rank[:, k] < k_n)
            s = [np.where(use, s[a] + d[:, a], s[a]) for a in range(3)]
        present = pres.sum(1)
        n_s, n_n = np.minimum(present, k_s), np.minimum(present, k_n)
        spacing = np.where(n_s > 0, np.sqrt(ssum / np.maximum(n_s, 1).astype(T)), T(0)).astype(T)
        degenerate = n_n < 2
        fn = (n_n + 1).astype(T)
        m = [s[a] / fn for a in range(3)]
        e = [T(0) - m[a] for a in range(3)]
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        acc = [e[a] * e[b] for a, b in pairs]
        for k in range(K):
            use = pres[:, k] & (rank[:, k] < k_n)
            e = [delta[:, k, a] - m[a] for a in range(3)]
            acc = [np.where(use, acc[i] + e[a] * e[b], acc[i]) for i, (a, b) in enumerate(pairs)]
        cov6 = np.stack([np.where(degenerate, T(0), x / fn) for x in acc], 1).astype(T)
        lam, V = jacobi(cov6, dtype=T)
        u = V[:, :, 0]
        ln = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        n = u / ln[:, None]
        if orient_to is not None:
            o = np.asarray(orient_to, F32).astype(T)
            flip = (n[:, 0] * (pts[:, 0] - o[0]) + n[:, 1] * (pts[:, 1] - o[1])) + n[:, 2] * (pts[:, 2] - o[2]) < 0
        else:
            lead = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
            flip = lead < 0
        n = np.where(flip[:, None], -n, n)
        w = V[:, :, 2]
        la = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        ea = w / la[:, None]
        b = np.stack([n[:, 1] * ea[:, 2] - n[:, 2] * ea[:, 1], n[:, 2] * ea[:, 0] - n[:, 0] * ea[:, 2],
                      n[:, 0] * ea[:, 1] - n[:, 1] * ea[:, 0]], 1)
        R = np.stack([ea, b, n], 2)                         # R[:, i, 0] = a_i, R[:, i, 1] = b_i, R[:, i, 2] = n_i
        quat = _quaternion(R, T)
    ident = np.array([1, 0, 0, 0], T)
    lam = np.where(degenerate[:, None], T(0), lam).astype(T)
    n = np.where(degenerate[:, None], np.array([0, 0, 1], T), n).astype(T)
    quat = np.where(degenerate[:, None], ident, quat).astype(T)
    return Geometry(spacing, cov6, lam, n, quat, degenerate)


def _quaternion(R, T):
    R00, R01, R02, R10, R11, R12, R20, R21, R22 = (R[:, i, j] for i in range(3) for j in range(3))
    tr = (R00 + R11) + R22
    w0 = np.sqrt(tr + T(1)) * T(2)
    q0 = (w0 / T(4), (R21 - R12) / w0, (R02 - R20) / w0, (R10 - R01) / w0)
    w1 = np.sqrt(((T(1) + R00) - R11) - R22) * T(2)
    q1 = ((R21 - R12) / w1, w1 / T(4), (R01 + R10) / w1, (R02 + R20) / w1)
    w2 = np.sqrt(((T(1) + R11) - R00) - R22) * T(2)
    q2 = ((R02 - R20) / w2, (R01 + R10) / w2, w2 / T(4), (R12 + R21) / w2)
    w3 = np.sqrt(((T(1) + R22) - R00) - R11) * T(2)
    q3 = ((R10 - R01) / w3, (R02 + R20) / w3, (R12 + R21) / w3, w3 / T(4))
    b0, b1, b2 = tr > 0, (R00 > R11) & (R00 > R22), R11 > R22
    q = [np.where(b0, q0[k], np.where(b1, q1[k], np.where(b2, q2[k], q3[k]))) for k in range(4)]
    lq = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [x / lq for x in q]
    neg = q[0] < 0
    return np.stack([np.where(neg, -x, x) for x in q], 1)


def quat_to_matrix(q):
    """the rotation the rasterizer builds from (r, x, y, z), float64 (include/gsr.h, the density-control section)"""
    r, x, y, z = (np.asarray(q, np.float64)[:, k] for k in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                     np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                     np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def cov_matrix(cov6):
    c = np.asarray(cov6, np.float64)
    return np.stack([np.stack([c[:, 0], c[:, 1], c[:, 2]], 1), np.stack([c[:, 1], c[:, 3], c[:, 4]], 1),
                     np.stack([c[:, 2], c[:, 4], c[:, 5]], 1)], 1)


def eigh64(cov6):
    """(eigenvalues ascending [P,3], eigenvectors as columns [P,3,3]) of the float32 cov6 in float64"""
    return np.linalg.eigh(cov_matrix(cov6))


def angle_deg(a, b):
    """the angle between the LINES of a and b (a normal's sign is a convention), degrees; from the cross product as well, so that
    a small angle keeps its digits (acos of a float32 dot product cannot show less than 0.03 degrees)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1))))


def handmade_lists(P, K, seed):
    """lists no search would write: -1 in the middle, indices out of range, repeats, the point itself, short and empty rows"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, P, (P, K)).astype(np.int32)
    idx[rng.random((P, K)) < 0.15] = -1
    idx[rng.random((P, K)) < 0.05] = P
    idx[rng.random((P, K)) < 0.05] = -7
    idx[rng.random((P, K)) < 0.03] = 2 ** 31 - 1
    idx[rng.random((P, K)) < 0.03] = -2 ** 31
    idx[::11] = -1                                           # no neighbour at all
    idx[1::11, 1:] = -1                                      # one neighbour: a degenerate row with a spacing
    idx[2::11, 0] = np.arange(P, dtype=np.int32)[2::11]      # the point itself
    return idx
