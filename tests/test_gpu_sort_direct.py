"""The radix sort (csrc/sort.hip) and the tile-range search (k_tile_ranges, csrc/binning.hip) against numpy, directly, through the
probes gsr_sort_probe / gsr_tile_ranges_probe -- at the digit widths, block counts, partial blocks, device counts and control
words that a rendered scene only reaches by luck, and on the depth sort's full-size blocks, which no scene below 16.7 M
Gaussian-views reaches at all.  Integer data, exact comparisons.  Cases and references: tests/sort_cases.py (checked on the host by
tests/test_cpu_sort_cases.py)."""
import numpy as np
import pytest
import torch

import sort_cases as S

pytestmark = pytest.mark.gpu

_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.uint64): np.int64}


def _dev(a, device):
    """an unsigned numpy array as the same-width signed tensor on the device (bit patterns)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED[a.dtype])).to(device)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _probe(N, keys_t, vals_t, **kw):
    """gsr_sort_probe, plus: the inputs come back untouched"""
    k0 = keys_t.clone()
    v0 = vals_t.clone() if vals_t is not None else None
    out = N.sort_probe(keys_t, vals_t, **kw)
    assert torch.equal(keys_t, k0) and (vals_t is None or torch.equal(vals_t, v0)), "the probe modified its inputs"
    return out


def _run_case(N, device, c):
    keys, vals = S.case_arrays(c)
    ko, vo, ctl = _probe(N, _dev(keys, device), None if vals is None else _dev(vals, device), cap=c.n, end_bit=c.end_bit,
                         small_blocks=S.KINDS[c.kind][1])
    assert ctl is None
    try:
        S.check_sort(keys, vals, c.end_bit, _host(ko, keys.dtype), _host(vo, np.uint32)[:c.n])
    except AssertionError as e:
        raise AssertionError("%s (blocks %d, padded %d, digit widths %s): %s" % (c.name, c.nblk, c.nblk_pad, c.widths, e)) from None


# ---- digit widths: every k_radix_scatter<BITS> of both key types, and the half-size variant -----------------------------------------
_WIDTHS = [(kind, e) for kind in ("u32", "u16", "small") for e in sorted(S.width_cases(kind))]


@pytest.mark.parametrize("kind,end_bit", _WIDTHS, ids=["%s-%d" % w for w in _WIDTHS])
def test_digit_widths(gpu_device, kind, end_bit):
    from diff_gaussian_rasterization import _native as N
    for c in S.width_cases(kind)[end_bit]:
        _run_case(N, gpu_device, c)


# ---- sizes: partial blocks, wave and segment edges, the workgroup -> block map's group change, the row scan's second lap ------------
_SIZES = [(kind, n) for kind in ("u32", "u16", "small") for n in S.size_list(kind)]


@pytest.mark.parametrize("kind,n", _SIZES, ids=["%s-%d" % s for s in _SIZES])
def test_sizes(gpu_device, kind, n):
    from diff_gaussian_rasterization import _native as N
    for c in S.size_cases(kind)[n]:
        _run_case(N, gpu_device, c)


# ---- device counts and batches ---------------------------------------------------------------------------------------------------
def _pack(arrays, stride, dtype):
    """views `stride` bytes apart in one buffer"""
    item = np.dtype(dtype).itemsize
    buf = np.zeros(len(arrays) * stride // item, dtype=dtype)
    for v, a in enumerate(arrays):
        buf[v * stride // item: v * stride // item + a.shape[0]] = a
    return buf


def _view(buf, v, stride, n):
    item = buf.dtype.itemsize
    return buf[v * stride // item: v * stride // item + n]


@pytest.mark.parametrize("kind", ["u32", "u16", "small"])
@pytest.mark.parametrize("given_vals", [False, True], ids=["iota", "vals"])
def test_device_counts_in_a_batch(gpu_device, kind, given_vals):
    """V = 4 with device counts [n0, 0, cap + 1000, 1]: a partial view, an empty one, one whose count exceeds the capacity and a
    single element, at a view stride that is a multiple of 256 B but not of a sort block"""
    from diff_gaussian_rasterization import _native as N
    key_bits, small, tile = S.KINDS[kind]
    kdt = np.uint16 if key_bits == 16 else np.uint32
    cap, e = 10007, S.SIZE_END_BIT[kind]
    stride = (cap * 4 + 255) // 256 * 256 + 256
    assert stride % 256 == 0 and stride % (tile * 4) != 0 and stride % (tile * 2) != 0
    counts = [9001, 0, cap + 1000, 1]
    keys = [S.make_keys(cap, e, key_bits, p, 40 + v) for v, p in enumerate(("ties", "highbits", "highbits", "ties"))]
    vals = [S.make_vals(cap, 40 + v) for v in range(4)] if given_vals else None
    cnt = np.zeros((4, 3), dtype=np.int64)     # the counts have a stride of their own (24 B)
    cnt[:, 0] = counts
    cnt[:, 1:] = 123456789
    ko, vo, _ = _probe(N, _dev(_pack(keys, stride, kdt), gpu_device), None if vals is None else _dev(_pack(vals, stride, np.uint32), gpu_device),
                       cap=cap, end_bit=e, V=4, stride=stride, counts=torch.from_numpy(cnt).to(gpu_device), small_blocks=small)
    ko, vo = _host(ko, kdt), _host(vo, np.uint32)
    for v in range(4):
        n = min(counts[v], cap)
        S.check_sort(keys[v][:n], None if vals is None else vals[v][:n], e, _view(ko, v, stride, n), _view(vo, v, stride, n))


@pytest.mark.parametrize("kind", ["u32", "u16", "small"])
def test_host_count_batch_and_empty_call(gpu_device, kind):
    from diff_gaussian_rasterization import _native as N
    key_bits, small, tile = S.KINDS[kind]
    kdt = np.uint16 if key_bits == 16 else np.uint32
    cap, e = 4097, S.SIZE_END_BIT[kind]
    stride = (cap * 4 + 255) // 256 * 256 + 512
    keys = [S.make_keys(cap, e, key_bits, "ties", 50 + v) for v in range(2)]
    kt = _dev(_pack(keys, stride, kdt), gpu_device)
    ko, vo, _ = _probe(N, kt, None, cap=cap, end_bit=e, V=2, stride=stride, small_blocks=small)    # n_dev NULL: cap elements each
    for v in range(2):
        S.check_sort(keys[v], None, e, _view(_host(ko, kdt), v, stride, cap), _view(_host(vo, np.uint32), v, stride, cap))
    # cap == 0: OK, and neither output is touched
    sk = torch.full_like(kt, 0x5A5A if key_bits == 16 else 0x5A5A5A5A)
    sv = torch.full((kt.numel(),), 0x3C3C3C3C, dtype=torch.int32, device=gpu_device)
    sk0, sv0 = sk.clone(), sv.clone()
    flags = (N.SORT_KEY16 if key_bits == 16 else 0) | (N.SORT_SMALL_BLOCKS if small else 0)
    with torch.cuda.device(gpu_device):
        rc = N.lib.gsr_sort_probe(kt.data_ptr(), None, stride, None, 0, 2, 0, e, flags, sk.data_ptr(), sv.data_ptr(), None,
                                  N._stream_handle(gpu_device))
    torch.cuda.synchronize(gpu_device)
    assert rc == 0 and torch.equal(sk, sk0) and torch.equal(sv, sv0)


# ---- depth control: control words, skipped passes, per-view result buffers, on both block sizes ------------------------------------
_DEPTH = [(small, name) for small in (False, True) for name in S.DEPTH_NAMES]
_DEPTH_CACHE = {}


def _depth_case(small, name):
    if small not in _DEPTH_CACHE:   # (built once per block size, on first use)
        _DEPTH_CACHE[small] = {c.name.split("-", 1)[1]: c for c in S.depth_cases(small)}
    return _DEPTH_CACHE[small][name]


@pytest.mark.parametrize("small,name", _DEPTH, ids=["%s-%s" % ("small" if s else "full", n) for s, n in _DEPTH])
def test_depth_control(gpu_device, small, name):
    from diff_gaussian_rasterization import _native as N
    c = _depth_case(small, name)
    ko, vo, ctl = _probe(N, _dev(c.keys, gpu_device), None, cap=c.n, end_bit=32, small_blocks=small, depth_ctl=True)
    ctl = _host(ctl, np.uint32)[0]
    print("%s: n %d, blocks %d (padded %d); control words %s, expected (%#x, %d, %d)" % (c.name, c.n, c.nblk, c.nblk_pad, ctl.tolist(), c.base, c.bits, c.passes))
    assert (int(ctl[0]), int(ctl[1]), int(ctl[2])) == (c.base, c.bits, c.passes), c.name
    S.check_depth(c.keys, _host(ko, np.uint32), _host(vo, np.uint32)[:c.n], ctl)


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
def test_depth_control_views_end_in_different_buffers(gpu_device, small):
    """one call, three views needing 1, 3 and 4 passes: each view's result is read from the buffer its own pass count names"""
    from diff_gaussian_rasterization import _native as N
    views = S.depth_batch(small)
    n = views[0].n
    stride = (n * 4 + 255) // 256 * 256 + 256
    ko, vo, ctl = _probe(N, _dev(_pack([c.keys for c in views], stride, np.uint32), gpu_device), None, cap=n, end_bit=32, V=3,
                         stride=stride, small_blocks=small, depth_ctl=True)
    ko, vo, ctl = _host(ko, np.uint32), _host(vo, np.uint32), _host(ctl, np.uint32)
    assert [int(w) for w in ctl[:, 2]] == [1, 3, 4]
    for v, c in enumerate(views):
        S.check_depth(c.keys, _view(ko, v, stride, n), _view(vo, v, stride, n), ctl[v])


# ---- tile ranges ------------------------------------------------------------------------------------------------------------------
def _ranges(N, device, keys, counts, cap, T, kdt, V=1, stride=0):
    kt = _dev(np.ascontiguousarray(keys if keys.shape[0] else np.zeros(1), dtype=kdt), device)
    cnt = torch.tensor([[int(c), -1] for c in counts], dtype=torch.int64, device=device)
    r = N.tile_ranges_probe(kt, cnt, cap, T, V=V, stride=stride)
    torch.cuda.synchronize(device)
    return r.cpu().numpy()


_RANGE_PARAMS = [(k, T) for k in ("u16", "u32") for T in S.RANGE_T] + [("u32", 70000)]


@pytest.mark.parametrize("key,T", _RANGE_PARAMS, ids=["%s-T%d" % p for p in _RANGE_PARAMS])
def test_tile_ranges(gpu_device, key, T):
    from diff_gaussian_rasterization import _native as N
    kdt = np.uint16 if key == "u16" else np.uint32
    for c in S.range_cases(T):
        try:
            S.check_ranges(c.keys, c.n, T, _ranges(N, gpu_device, c.keys, [c.n], c.n, T, kdt)[0])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (c.name, e)) from None


@pytest.mark.parametrize("key", ["u16", "u32"])
def test_tile_ranges_counts(gpu_device, key):
    """a device count above the capacity, and V = 3 with counts [n, 0, 1] on views a stride apart"""
    from diff_gaussian_rasterization import _native as N
    kdt = np.uint16 if key == "u16" else np.uint32
    T, n = 511, 8193
    c = S.range_case(T, n, "sample_edges")
    S.check_ranges(c.keys, n, T, _ranges(N, gpu_device, c.keys, [n + 1000], n, T, kdt)[0])
    S.check_ranges(c.keys, 5000, T, _ranges(N, gpu_device, c.keys, [1 << 40], 5000, T, kdt)[0])
    views = [S.range_case(T, n, lay, seed=3).keys for lay in ("gaps", "random", "last_tile")]
    stride = (n * 4 + 255) // 256 * 256 + 256
    r = _ranges(N, gpu_device, _pack([v.astype(kdt) for v in views], stride, kdt), [n, 0, 1], n, T, kdt, V=3, stride=stride)
    for v, cnt in enumerate((n, 0, 1)):
        S.check_ranges(views[v], cnt, T, r[v])


_RANGE_LIMIT = S.RANGE_MAX_SAMPLES * S.RANGE_SAMPLE   # 33.5 M keys


@pytest.mark.parametrize("n", [_RANGE_LIMIT, _RANGE_LIMIT + 1], ids=["at-the-sample-limit", "plain-search"])
def test_tile_ranges_either_side_of_the_sample_limit(gpu_device, n):
    """8192 samples still fit the LDS table; one key more and the kernel takes the plain binary search.  16-bit keys made and
    sorted on the device, reference from the copied-back array."""
    from diff_gaussian_rasterization import _native as N
    T = 8160
    g = torch.Generator(device=gpu_device)
    g.manual_seed(n)
    keys = torch.randint(0, T, (n,), dtype=torch.int16, device=gpu_device, generator=g)
    keys[:3] = 0
    keys, _ = torch.sort(keys)
    cnt = torch.tensor([[n]], dtype=torch.int64, device=gpu_device)
    r = N.tile_ranges_probe(keys, cnt, n, T)
    torch.cuda.synchronize(gpu_device)
    S.check_ranges(keys.cpu().numpy(), n, T, r.cpu().numpy()[0])
