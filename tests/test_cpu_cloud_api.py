"""The point-cloud neighbourhood entries (include/gsr.h gsr_knn_scratch_bytes / gsr_knn / gsr_cloud_geometry) and pcrender.cloud as far as
they can be reached without a GPU: the exported symbols and their arguments, the header's formulas, the refusals that precede any HIP
call, in their order (stand-in pointers that are never followed), the size query, the Python side's refusals, and
gaussians_from_points' argument handling on CPU tensors."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import cloud_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, Cc, D, E, Fp, G, Hh = (0x1000 * k for k in range(1, 9))          # stand-ins for device arrays (never followed)
SYMS = ("gsr_knn_scratch_bytes", "gsr_knn", "gsr_cloud_geometry")
INVALID, CAPACITY = -1, -3


def _native():
    from diff_gaussian_rasterization import _native as N
    return N


def test_symbols_are_exported_declared_and_bound():
    N = _native()
    lib = ctypes.CDLL(N.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "gsr.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = {}
    for sym in SYMS:
        assert hasattr(lib, sym) and sym in N.SYMBOLS and sym in N._DECL, sym
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)" % sym, header)
        assert m, "include/gsr.h does not declare %s" % sym
        names[sym] = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert len(names[sym]) == len(N._DECL[sym][1]), sym
    assert names[SYMS[0]] == ["P", "K"] and N._DECL[SYMS[0]][0] is ctypes.c_size_t
    assert names[SYMS[1]] == ["P", "points", "K", "idx", "d2", "scratch", "scratch_bytes", "stream"]
    assert names[SYMS[2]] == ["P", "points", "K", "knn_idx", "k_s", "k_n", "orient_to", "spacing", "cov6", "eigenvalues", "normals",
                              "rotations", "stream"]
    assert N._DECL[SYMS[1]][1][6] is ctypes.c_size_t
    assert N.CLOUD_OUTPUTS == tuple(names[SYMS[2]][7:12]) and N.CLOUD_MAX_K == R.MAX_K == 32
    assert int(re.search(r"#define GSR_CLOUD_JACOBI_SWEEPS (\d+)", header).group(1)) == R.SWEEPS
    # the header states the definition formula by formula, and the contract
    doc = text[text.index("Point-cloud neighbourhoods: exact k nearest neighbours"):text.index("#define GSR_CLOUD_JACOBI_SWEEPS")]
    for phrase in ("d2(i, j) = (dx dx + dy dy) + dz dz", "smallest (d2, j) in lexicographic order", "ties go to the lower", "idx = -1 and d2 = +inf",
                   "A point with a non-finite coordinate is absent", "K in 1..32, 1 <= P < 2^30", "g_a = max(lo_a - q_a, q_a - hi_a, 0)",
                   "bound = (g_x g_x + g_y g_y) + g_z g_z", "strictly greater", "rounding is monotone", "at most once per run",
                   "its contents on entry do not matter", "Nothing is read back from the device, no host wait is made, nothing is",
                   "There are no atomics", "two calls give the same bits", "GSR_ERR_CAPACITY",
                   "spacing = sqrtf(sum / (float)n_s)", "3DGS's initial scale", "m = s / (float)n", "e_self = 0 - m",
                   "C_ab = acc_ab / (float)n", "(C_xx, C_xy, C_xz, C_yy, C_yz, C_zz)", "DEGENERATE ROW", "No output of a degenerate row is NaN",
                   "theta = (A_qq - A_pp) / (2 A_pq)", "t = sgn / (|theta| + sqrtf(theta theta + 1))", "c = 1 / sqrtf(t t + 1)", "s = t c",
                   "(0, 1), (1, 2), (0, 1)", "no closed-form trigonometric solver", "n . (p - orient_to) >= 0",
                   "first non-zero component is negative", "b = n x a", "r >= 0", "sqrt of (lambda_2, lambda_1, lambda_0)", "HOST",
                   "Every output pointer is optional"):
        assert phrase in doc, phrase
    assert list(inspect.signature(N.knn).parameters) == ["points", "K", "want_d2"]
    assert list(inspect.signature(N.cloud_geometry).parameters) == ["points", "knn_idx", "k_s", "k_n", "orient_to", "want"]
    build = open(os.path.join(ROOT, "gaussian-pcloud-render_amd", "build.py")).read()
    assert '"cloud_geometry"' in build[build.index("UNITS ="):build.index("FLAGS =")]
    for f in ("cloud_geometry.hip", "cloud_geometry.hpp"):
        assert os.path.exists(os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc", f))
    # the hot path has no atomics and no device -> host copy of its own
    src = open(os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc", "cloud_geometry.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("atomic", "hipMemcpy", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize"):
        assert word not in code, word
    assert "launch_radix_sort_pairs" in code and "k_radix" not in code          # the library's sort, not a second one


def test_size_query_is_monotone_a_multiple_of_256_and_zero_for_refused_sizes():
    f = _native().lib.gsr_knn_scratch_bytes
    prev = 0
    for P in (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 70001, 800_000, 2_000_000, (1 << 30) - 1):
        for K in (1, 3, 16, 32):
            n = f(P, K)
            assert n >= prev and n > 0 and n % 256 == 0 and n >= 32 * P, (P, K, n)
            prev = n
        prev = f(P, 1)
    assert all(f(P, 32) >= f(P, 1) for P in (1, 4097, 800_000))
    # about 33 B per point: two key and two index arrays, the sorted 16-B records and the boxes
    assert 32 * 800_000 < f(800_000, 16) < 36 * 800_000
    for P, K in ((0, 3), (-1, 3), (1 << 30, 3), (2147483647, 3), (-2147483648, 3), (1000, 0), (1000, 33), (1000, -1)):
        assert f(P, K) == 0, (P, K)


def test_knn_refusals_before_any_hip_call_in_their_order():
    lib = _native().lib

    def call(P=1000, K=16, points=A, idx=B, d2=Cc, scratch=0x10000, scratch_bytes=None):
        nbytes = lib.gsr_knn_scratch_bytes(P, K) if scratch_bytes is None else scratch_bytes
        return lib.gsr_knn(P, points, K, idx, d2, scratch, nbytes, None), lib.gsr_last_error()

    # 1. the sizes, whatever else is wrong
    for P, K in ((0, 16), (-5, 16), (1 << 30, 16), (2147483647, 1), (1000, 0), (1000, 33), (1000, -2)):
        rc, err = call(P=P, K=K, points=None, scratch_bytes=0)
        assert rc == INVALID and b"knn" in err and b"bad sizes" in err, (P, K, err)
    # 2. the pointers (a NULL d2 is "not wanted", never refused), before the scratch size
    for kw in (dict(points=None), dict(idx=None), dict(scratch=None)):
        rc, err = call(scratch_bytes=0, **kw)
        assert rc == INVALID and b"knn" in err and b"is NULL" in err, (kw, err)
    # 3. the scratch, with the size needed
    need = lib.gsr_knn_scratch_bytes(1000, 16)
    for d2 in (Cc, None):
        rc, err = call(d2=d2, scratch_bytes=need - 1)
        assert rc == CAPACITY and b"knn" in err and str(need).encode() in err, err
    rc, err = call(scratch_bytes=0)
    assert rc == CAPACITY


def test_cloud_geometry_refusals_before_any_hip_call_in_their_order():
    lib = _native().lib
    outs = ("spacing", "cov6", "eigenvalues", "normals", "rotations")
    host3 = (ctypes.c_float * 3)(0, 0, 0)

    def call(P=1000, K=16, k_s=3, k_n=16, points=A, knn_idx=B, orient_to=None, **null):
        ptr = dict(zip(outs, (Cc, D, E, Fp, G)))
        ptr.update({k: None for k in null})
        return lib.gsr_cloud_geometry(P, points, K, knn_idx, k_s, k_n, orient_to, *[ptr[k] for k in outs], None), lib.gsr_last_error()

    none = {k: 1 for k in outs}
    # 1. the sizes, whatever else is wrong
    for kw in (dict(P=0), dict(P=-1), dict(P=1 << 30), dict(K=0), dict(K=33), dict(k_s=0), dict(k_s=17), dict(k_n=0), dict(k_n=17), dict(k_n=-3)):
        rc, err = call(points=None, **kw, **none)
        assert rc == INVALID and b"cloud_geometry" in err and b"bad sizes" in err, (kw, err)
    # 2. the inputs, before the outputs
    for kw in (dict(points=None), dict(knn_idx=None)):
        rc, err = call(orient_to=ctypes.addressof(host3), **kw, **none)
        assert rc == INVALID and b"cloud_geometry" in err and b"is NULL" in err, (kw, err)
    # 3. nothing to compute
    rc, err = call(**none)
    assert rc == INVALID and b"cloud_geometry" in err and b"no output" in err, err


def test_python_wrappers_refuse_cpu_tensors_and_malformed_arguments():
    N = _native()
    p = torch.rand(40, 3)
    idx = torch.zeros((40, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.knn(p, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.knn(p, 1, want_d2=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.cloud_geometry(p, idx)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.cloud_geometry(p, idx, k_s=9, k_n=2, orient_to=torch.zeros(3), want=("normals",))       # k_s is clipped to K
    for bad in (p.double(), torch.rand(40, 4), torch.rand(3, 40).t(), torch.rand(0, 3), torch.rand(40), p.half()):
        with pytest.raises(ValueError):
            N.knn(bad, 8)
        with pytest.raises(ValueError):
            N.cloud_geometry(bad, idx)
    for K in (0, 33, -1):
        with pytest.raises(ValueError):
            N.knn(p, K)
    for bad in (idx.long(), torch.zeros((39, 8), dtype=torch.int32), torch.zeros((8, 40), dtype=torch.int32).t(),
                torch.zeros((40, 33), dtype=torch.int32), torch.zeros((40,), dtype=torch.int32), torch.zeros((40, 0), dtype=torch.int32)):
        with pytest.raises(ValueError):
            N.cloud_geometry(p, bad)
    for kw in (dict(k_s=0), dict(k_n=0), dict(k_n=9), dict(want=()), dict(want=("normals", "tangents")), dict(orient_to=(0.0, 1.0)),
               dict(orient_to=torch.zeros(4))):
        with pytest.raises(ValueError):
            N.cloud_geometry(p, idx, **kw)


def test_pcrender_cloud_surface_and_argument_handling_on_the_host():
    from pcrender import cloud
    assert list(inspect.signature(cloud.knn).parameters) == ["points", "K", "want_d2"]
    assert list(inspect.signature(cloud.cloud_geometry).parameters) == ["points", "knn_idx", "k_s", "k_n", "orient_to", "want"]
    sig = inspect.signature(cloud.gaussians_from_points)
    assert list(sig.parameters)[:10] == ["points", "colors", "mode", "K", "k_s", "scale_factor", "voxelized", "log_scales", "thickness", "offset"]
    assert (sig.parameters["mode"].default, sig.parameters["K"].default, sig.parameters["k_s"].default,
            sig.parameters["log_scales"].default) == ("isotropic", 16, 3, False)
    assert cloud.Neighbours._fields == ("idx", "d2") and cloud.CloudGeometry._fields == _native().CLOUD_OUTPUTS
    assert cloud.MODES == ("isotropic", "surfel")
    s = torch.tensor([0.0, 2.0, 4.0, 0.0])
    assert float(cloud.mean_spacing(s)) == 3.0 and float(cloud.mean_spacing(torch.zeros(3))) == 0.0
    p, c = torch.rand(30, 3), torch.rand(30, 3)
    for kw in (dict(mode="disc"), dict(thickness=0.0), dict(thickness=-1.0)):
        with pytest.raises(ValueError):
            cloud.gaussians_from_points(p, c, **kw)
    for bad in ((torch.rand(30, 2), c), (p, torch.rand(29, 3)), (p, torch.rand(30, 4)), (torch.rand(30), c)):
        with pytest.raises(ValueError):
            cloud.gaussians_from_points(*bad)
    for mode in cloud.MODES:
        with pytest.raises(RuntimeError, match="no CPU path"):
            cloud.gaussians_from_points(p, c, mode=mode)
        with pytest.raises(RuntimeError, match="no CPU path"):
            cloud.gaussians_from_points(p * 100 + 512, c, mode=mode, voxelized=True, scale_factor=256.0, log_scales=True, K=99)
    # what exists today stays as it is
    from pcrender import raster_passes as rp
    assert list(inspect.signature(rp.simple_primitives).parameters) == ["points", "colors", "sigma", "scale_factor", "voxelized", "offset"]
