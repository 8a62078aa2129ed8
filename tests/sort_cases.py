"""Seeded cases and exact host references for the direct tests of the radix sort (csrc/sort.hip) and the tile-range search
(k_tile_ranges, csrc/binning.hip), reached through the probes gsr_sort_probe / gsr_tile_ranges_probe.

Everything here is integer data and numpy: the GPU tests compare with assert_array_equal, no tolerances.  Each case carries the
edge it is meant to hit as data (block count, padded block count, pass widths, control words), and tests/test_cpu_sort_cases.py
checks on the host that the generators really produce those edges and that the checkers reject known-bad outputs."""
from collections import namedtuple

import numpy as np

RADIX_BITS = 8
TILE = 4096          # keys per full-size sort block (common.hpp RS_TILE)
TILE_SMALL = 2048    # keys per half-size sort block (RS_TILE_SMALL)
HIST_GROUP = 16      # blocks per 64-B line of the count matrix; the scatter's workgroup -> block map works on 8 * HIST_GROUP blocks
CULLED = 0xFFFFFFFF
RANGE_SAMPLE = 4096        # binning.hip: every RANGE_SAMPLE-th key is staged in LDS ...
RANGE_MAX_SAMPLES = 8192   # ... up to this many; longer lists take the plain search
RANGE_TILES_PER_WG = 255


# ---- the sort's own arithmetic, restated ---------------------------------------------------------------------------------------
def pass_widths(end_bit):
    """digit widths of launch_radix_sort_pairs: ceil(end_bit / 8) passes, the bits split evenly, wider digits first"""
    npass = (end_bit + RADIX_BITS - 1) // RADIX_BITS
    out, shift = [], 0
    for p in range(npass):
        bits = (end_bit - shift + (npass - p) - 1) // (npass - p)
        out.append(bits)
        shift += bits
    return out


def blocks(n, tile):
    return (n + tile - 1) // tile


def hist_stride(n, tile):
    """padded block count of the count matrix (common.hpp sort_hist_stride)"""
    return (blocks(n, tile) + 15) // 16 * 16


def depth_sort_passes(bits):
    return (bits + RADIX_BITS - 1) // RADIX_BITS


def wg_to_block(wg):
    """k_radix_scatter's workgroup -> sort block map"""
    xcd, r = wg & 7, wg >> 3
    return ((r // HIST_GROUP) * 8 + xcd) * HIST_GROUP + r % HIST_GROUP


# ---- plain sort ---------------------------------------------------------------------------------------------------------------
KINDS = {   # name -> (key bits, small blocks, tile)
    "u32": (32, False, TILE),
    "u16": (16, False, TILE),
    "small": (32, True, TILE_SMALL),
}
PATTERNS = ("ties", "equal", "ascending", "descending", "alternating", "topbit", "highbits")

SortCase = namedtuple("SortCase", "name kind n end_bit pattern given_vals seed nblk nblk_pad widths")


def sort_case(kind, n, end_bit, pattern, given_vals, seed=0):
    tile = KINDS[kind][2]
    return SortCase("%s-n%d-b%d-%s-%s" % (kind, n, end_bit, pattern, "vals" if given_vals else "iota"), kind, n, end_bit, pattern,
                    given_vals, seed, blocks(n, tile), hist_stride(n, tile), tuple(pass_widths(end_bit)))


def make_keys(n, end_bit, key_bits, pattern, seed):
    """uint32 / uint16 keys of one pattern; only "highbits" (and "ties" below 12 bits) sets bits at and above end_bit"""
    rng = np.random.default_rng([seed, n, end_bit, key_bits, PATTERNS.index(pattern)])
    mask = (1 << end_bit) - 1
    full = (1 << key_bits) - 1
    i = np.arange(n, dtype=np.uint64)
    if pattern == "ties":
        k = (rng.integers(0, 1 << 32, n, dtype=np.uint64) >> np.uint64(8)) % np.uint64(3001)
    elif pattern == "equal":
        k = np.full(n, 0x2A5 & mask, dtype=np.uint64)
    elif pattern == "ascending":
        k = i * np.uint64(mask + 1) // np.uint64(max(n, 1))
    elif pattern == "descending":
        k = np.uint64(mask) - i * np.uint64(mask + 1) // np.uint64(max(n, 1))
    elif pattern == "alternating":
        k = np.where(i & np.uint64(1), np.uint64(mask), np.uint64(mask >> 1))
    elif pattern == "topbit":
        k = np.uint64(0x155 & (mask >> 1)) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(end_bit - 1))
    elif pattern == "highbits":
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    else:
        raise ValueError(pattern)
    return (k & np.uint64(full)).astype(np.uint16 if key_bits == 16 else np.uint32)


def make_vals(n, seed):
    """arbitrary 32-bit values with repeats (the sort must carry them, not rebuild them)"""
    rng = np.random.default_rng([seed, n, 77])
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def case_arrays(c):
    keys = make_keys(c.n, c.end_bit, KINDS[c.kind][0], c.pattern, c.seed)
    return keys, (make_vals(c.n, c.seed) if c.given_vals else None)


def sort_reference(keys, vals, end_bit):
    """(keys, values) after a stable sort on key bits [0, end_bit); vals None: index values.  All key bits come back intact."""
    mask = keys.dtype.type((1 << end_bit) - 1)
    order = np.argsort(keys & mask, kind="stable")
    v = np.arange(keys.shape[0], dtype=np.uint32) if vals is None else vals
    return keys[order], v[order]


def check_sort(keys, vals, end_bit, keys_out, vals_out):
    ek, ev = sort_reference(keys, vals, end_bit)
    np.testing.assert_array_equal(np.asarray(vals_out, dtype=np.uint32), ev)
    np.testing.assert_array_equal(np.asarray(keys_out, dtype=keys.dtype), ek)


WIDTH_N = 10007   # two full blocks and a tail of full-size blocks: both paths of the 16-bit histogram


def width_cases(kind):
    """{end_bit: [cases]}: every digit width of a key type at n = 10007, every pattern, given and index values"""
    ends = {"u32": range(1, 33), "u16": range(1, 17), "small": (8, 16, 24, 32)}[kind]
    return {e: [sort_case(kind, WIDTH_N, e, p, g) for p in PATTERNS for g in (False, True)] for e in ends}


SIZE_END_BIT = {"u32": 13, "u16": 13, "small": 32}


def size_list(kind):
    tile = KINDS[kind][2]
    ns = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192]
    if kind == "small":
        ns += [2047, 2048, 2049]
    ns += [128 * tile - 1, 128 * tile, 128 * tile + 1]   # the scatter's workgroup -> block map changes group at block 128
    ns += [256 * tile + 1]                               # 257 blocks: nblk_pad = 272, the row scan's second lap
    return sorted(ns)


def size_cases(kind):
    """{n: [cases]}: every pattern with index values, "ties" and "highbits" with given values as well"""
    e = SIZE_END_BIT[kind]
    return {n: [sort_case(kind, n, e, p, False) for p in PATTERNS] + [sort_case(kind, n, e, p, True) for p in ("ties", "highbits")]
            for n in size_list(kind)}


# ---- depth sort (control words) ---------------------------------------------------------------------------------------------------
DepthCase = namedtuple("DepthCase", "name n small keys base bits passes nblk nblk_pad")


def expected_ctl(keys):
    """(base, bits, passes) the depth sort must report for these keys"""
    vis = keys[keys != CULLED]
    if vis.size == 0:
        base, bits = 0, 8
    else:
        base = int(vis.min()) & ~255
        bits = max(8, (int(vis.max()) - base).bit_length())
    return base, bits, depth_sort_passes(bits)


def _depth_case(name, small, keys):
    tile = TILE_SMALL if small else TILE
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    base, bits, passes = expected_ctl(keys)
    return DepthCase(name, keys.shape[0], small, keys, base, bits, passes, blocks(keys.shape[0], tile), hist_stride(keys.shape[0], tile))


def span_keys(n, bits, tile, seed, min_at=None, max_at=None, cull_every=16):
    """Keys whose visible span needs exactly `bits` key bits: the smallest visible key at index min_at (default: in the last,
    partial block), the largest at max_at (default: in the first block), ties in between, every cull_every-th key culled."""
    rng = np.random.default_rng([seed, n, bits, tile])
    base = 0x100 if bits == 32 else 0x3F123400
    lo = base + 0x37
    hi = 0xFFFFFFFE if bits == 32 else (base + 200 if bits == 8 else base + (1 << (bits - 1)) + 0x11)
    pool = lo + 1 + rng.integers(0, hi - lo - 1, 997, dtype=np.int64)   # strictly inside (lo, hi); 997 values: many ties
    k = pool[rng.integers(0, pool.size, n)].astype(np.uint32)
    if cull_every:
        k[5::cull_every] = CULLED
    min_at = n - 2 if min_at is None else min_at
    max_at = min(n - 1, 70) if max_at is None else max_at
    k[max_at] = hi
    k[min_at] = lo      # (n == 1: the one key is both)
    return k


DEPTH_NAMES = ("span8", "span9", "span16", "span17", "span24", "span25", "span32", "all-culled", "one-visible", "visible-equal",
               "ninth-culled", "258-blocks")


def depth_cases(small):
    """the cases of one block size, named "<full|small>-<DEPTH_NAMES[i]>" """
    tile = TILE_SMALL if small else TILE
    tag = "small" if small else "full"
    out = []
    n = 3 * tile + 5   # the smallest visible key in the last partial block, the largest in the first
    for bits in (8, 9, 16, 17, 24, 25, 32):
        out.append(_depth_case("%s-span%d" % (tag, bits), small, span_keys(n, bits, tile, 1)))
    m = tile + 17
    out.append(_depth_case(tag + "-all-culled", small, np.full(m, CULLED, dtype=np.uint32)))
    k = np.full(m, CULLED, dtype=np.uint32)
    k[tile + 3] = 0x40490FDB
    out.append(_depth_case(tag + "-one-visible", small, k))
    k = np.full(m, 0x3F800001, dtype=np.uint32)
    k[7::5] = CULLED
    out.append(_depth_case(tag + "-visible-equal", small, k))
    k = span_keys(m, 24, tile, 2, cull_every=0)
    k[::9] = CULLED
    out.append(_depth_case(tag + "-ninth-culled", small, k))
    # 258 blocks (nblk_pad = 272): the control workgroup's threads take a second lap over the per-block extremes (b += 256); the
    # smallest key sits in block 257, which only that lap reads
    n2 = 257 * tile + 1
    out.append(_depth_case(tag + "-258-blocks", small, span_keys(n2, 24, tile, 3, min_at=n2 - 1, max_at=11)))
    return out


def depth_batch(small):
    """three views of one call that need 1, 3 and 4 passes: their results end in different ping-pong buffers"""
    tile = TILE_SMALL if small else TILE
    n = 3 * tile + 5
    return [_depth_case("%s-batch-v%d" % ("small" if small else "full", v), small, span_keys(n, bits, tile, 10 + v))
            for v, bits in enumerate((8, 24, 32))]


def check_depth(keys, keys_out, vals_out, ctl):
    """The depth sort's contract: control words, a permutation, keys carried with their values, and the visible entries in
    stable key order.  Where culled entries land is immaterial and not looked at."""
    n = keys.shape[0]
    base, bits, passes = expected_ctl(keys)
    ctl = [int(x) & 0xFFFFFFFF for x in np.asarray(ctl).reshape(-1)[:4]]
    assert ctl[0] == base, "key base %#x, expected %#x" % (ctl[0], base)
    assert ctl[1] == bits, "key bits %d, expected %d" % (ctl[1], bits)
    assert ctl[2] == passes == depth_sort_passes(ctl[1]), "passes %d, expected %d" % (ctl[2], passes)
    vals_out = np.asarray(vals_out, dtype=np.uint32)
    keys_out = np.asarray(keys_out, dtype=np.uint32)
    assert vals_out.shape == (n,) and keys_out.shape == (n,)
    assert vals_out.max(initial=0) < max(n, 1), "a value is not an index"
    np.testing.assert_array_equal(np.sort(vals_out), np.arange(n, dtype=np.uint32), err_msg="values are not a permutation of 0..n-1")
    np.testing.assert_array_equal(keys_out, keys[vals_out], err_msg="keys do not travel with their values")
    vis_idx = np.nonzero(keys != CULLED)[0]
    expect = vis_idx[np.argsort(keys[vis_idx], kind="stable")].astype(np.uint32)
    np.testing.assert_array_equal(vals_out[keys_out != CULLED], expect, err_msg="visible entries are not in stable key order")


# ---- tile ranges --------------------------------------------------------------------------------------------------------------
RANGE_T = (1, 2, 254, 255, 256, 509, 510, 511, 8160)
RANGE_N = (0, 1, 4095, 4096, 4097, 8193, 100003)
RANGE_LAYOUTS = ("random", "tile0", "last_tile", "one_per_tile", "gaps", "sample_edges")

RangeCase = namedtuple("RangeCase", "name T n layout keys run_starts")


def _range_keys(T, n, layout, seed):
    """sorted tile ids (< T) of one layout as int64, or None where the layout does not exist at (T, n)"""
    rng = np.random.default_rng([seed, T, n, RANGE_LAYOUTS.index(layout)])
    if layout == "random":
        return np.sort(rng.integers(0, T, n))
    if layout == "tile0":
        return np.zeros(n, dtype=np.int64)
    if layout == "last_tile":
        return np.full(n, T - 1, dtype=np.int64)
    if layout == "one_per_tile":   # n = T by construction (made once per T)
        return np.arange(T, dtype=np.int64) if n == T else None
    if layout == "gaps":           # empty tiles at the front, in the middle and at the end
        if T < 8 or n == 0:
            return None
        allowed = np.concatenate([np.arange(T // 8, 3 * T // 8), np.arange(5 * T // 8, 7 * T // 8)])
        k = np.sort(allowed[rng.integers(0, allowed.size, n)])
        if n >= 2:
            k[0], k[-1] = allowed[0], allowed[-1]
        return k
    if layout == "sample_edges":   # tile runs start at 4096 j - 1, 4096 j and 4096 j + 1: just before, on and just after a sample
        js = list(range(1, (n - 1) // RANGE_SAMPLE + 1)) if n > 0 else []
        js = [j for j in js if RANGE_SAMPLE * j + 1 < n]
        room = (T - 1) // 3
        if not js or room == 0:
            return None
        if len(js) > room:         # fewer tiles than edges: keep the first and the last samples
            js = js[:(room + 1) // 2] + js[len(js) - room // 2:]
        starts = np.array(sorted(RANGE_SAMPLE * j + d for j in js for d in (-1, 0, 1)))
        step = np.zeros(n, dtype=np.int64)
        step[starts] = 1
        k = np.cumsum(step)
        return k + (T - 1 - k[-1]) // 2   # (ids end below T; some empty tiles either side when there is room)
    raise ValueError(layout)


def range_case(T, n, layout, seed=0):
    k = _range_keys(T, n, layout, seed)
    if k is None:
        return None
    assert k.shape == (n,) and (n == 0 or (0 <= k.min() and k.max() < T)) and bool(np.all(np.diff(k) >= 0))
    starts = np.nonzero(np.diff(k) != 0)[0] + 1 if n else np.zeros(0, dtype=np.int64)
    return RangeCase("T%d-n%d-%s" % (T, n, layout), T, n, layout, k, starts)


def range_cases(T):
    """every layout that exists at (T, n) for the n list, plus one pair per tile"""
    out = [range_case(T, n, lay) for n in RANGE_N for lay in RANGE_LAYOUTS if lay != "one_per_tile"]
    out.append(range_case(T, T, "one_per_tile"))
    return [c for c in out if c is not None]


def ranges_reference(keys, n, T):
    """int64 [T, 2]: (lower bound of t, lower bound of t + 1) in keys[:n], or (0, 0) for a tile without keys"""
    b = np.searchsorted(np.asarray(keys[:n]).astype(np.int64), np.arange(T + 1), "left")
    r = np.stack([b[:-1], b[1:]], axis=1).astype(np.int64)
    r[b[:-1] >= b[1:]] = 0
    return r


def check_ranges(keys, n, T, ranges):
    got = np.asarray(ranges).astype(np.int64) & 0xFFFFFFFF
    assert got.shape == (T, 2)
    np.testing.assert_array_equal(got, ranges_reference(keys, n, T))
