"""Host-side checks of tests/sort_cases.py: the generators produce the edges the GPU tests are meant to hit, and the checkers
reject known-bad outputs (this stands in for running broken kernels on the device)."""
import numpy as np
import pytest

import sort_cases as S


def test_pass_widths_split_the_bits_evenly_wider_first():
    assert S.pass_widths(13) == [7, 6] and S.pass_widths(12) == [6, 6] and S.pass_widths(32) == [8, 8, 8, 8]
    assert S.pass_widths(1) == [1] and S.pass_widths(17) == [6, 6, 5] and S.pass_widths(9) == [5, 4]
    seen = set()
    for e in range(1, 33):
        w = S.pass_widths(e)
        assert sum(w) == e and max(w) <= 8 and w == sorted(w, reverse=True)
        seen.update(w)
    assert seen == set(range(1, 9))          # uint32_t keys reach all eight scatter widths
    assert {b for e in range(1, 17) for b in S.pass_widths(e)} == set(range(1, 9))   # and so do uint16_t keys
    assert all(set(S.pass_widths(e)) == {8} for e in (8, 16, 24, 32))


def test_size_cases_hit_the_structural_edges():
    for kind, (_, small, tile) in S.KINDS.items():
        cases = S.size_cases(kind)
        ns = sorted(cases)
        for n in (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 128 * tile - 1, 128 * tile, 128 * tile + 1, 256 * tile + 1):
            assert n in ns
        if small:
            assert {2047, 2048, 2049} <= set(ns)
        by_n = {n: cs[0] for n, cs in cases.items()}
        assert by_n[128 * tile - 1].nblk == 128 and by_n[128 * tile].nblk == 128 and by_n[128 * tile + 1].nblk == 129
        assert by_n[256 * tile + 1].nblk == 257 and by_n[256 * tile + 1].nblk_pad == 272 > 256   # the row scan's second lap
        for n, cs in cases.items():
            assert {c.pattern for c in cs if not c.given_vals} == set(S.PATTERNS) and any(c.given_vals for c in cs)
            assert all(c.end_bit == S.SIZE_END_BIT[kind] and c.nblk == S.blocks(n, tile) for c in cs)
    full = {n: cs[0] for n, cs in S.size_cases("u32").items()}
    assert full[524289].nblk == 129 and full[524287].nblk == 128 and full[524288].nblk_pad == 128
    assert S.size_cases("u32")[4097][0].widths == (7, 6) and S.size_cases("small")[4097][0].widths == (8, 8, 8, 8)
    assert {262143, 262144, 262145} <= set(S.size_cases("small"))
    # block 128 is the first one served by the second group of workgroups, and the map is a permutation of each group
    assert S.wg_to_block(128) == 128 and S.wg_to_block(1) == 16 and S.wg_to_block(8) == 1
    assert sorted(S.wg_to_block(w) for w in range(256)) == list(range(256))


def test_width_cases_cover_every_width_and_both_histogram_paths():
    assert sorted(S.width_cases("u32")) == list(range(1, 33))
    assert sorted(S.width_cases("u16")) == list(range(1, 17))
    assert sorted(S.width_cases("small")) == [8, 16, 24, 32]
    for kind in S.KINDS:
        for e, cs in S.width_cases(kind).items():
            assert len(cs) == 2 * len(S.PATTERNS) and {(c.pattern, c.given_vals) for c in cs} == {(p, g) for p in S.PATTERNS for g in (False, True)}
            assert all(c.n == 10007 and c.widths == tuple(S.pass_widths(e)) for c in cs)
    c = S.width_cases("u16")[13][0]
    assert c.nblk == 3 and 10007 - 2 * S.TILE == 1815     # two full blocks (16-B loads) and a tail (2-B loads)


@pytest.mark.parametrize("key_bits", [16, 32])
def test_key_patterns_are_what_they_say(key_bits):
    n = 10007
    for e in (1, 5, 13, 16) + ((24, 32) if key_bits == 32 else ()):
        mask = (1 << e) - 1
        k = {p: S.make_keys(n, e, key_bits, p, 0).astype(np.int64) for p in S.PATTERNS}
        assert all(v.shape == (n,) and v.max() < (1 << key_bits) for v in k.values())
        assert len(np.unique(k["equal"])) == 1
        assert np.all(np.diff(k["ascending"]) >= 0) and k["ascending"][0] == 0 and k["ascending"][-1] == min(mask, (n - 1) * (mask + 1) // n)
        assert np.all(np.diff(k["descending"]) <= 0) and k["descending"][0] == mask
        a = k["alternating"]
        assert a[0] != a[1] and np.all(a[::2] == a[0]) and np.all(a[1::2] == a[1])
        t = k["topbit"]
        assert set(np.unique(t ^ t[0])) == {0, 1 << (e - 1)}            # differ in bit end_bit - 1 only, and do differ
        for p in ("equal", "ascending", "descending", "alternating", "topbit"):
            assert k[p].max() <= mask
        if e >= 12:
            assert k["ties"].max() <= 3000 and len(np.unique(k["ties"])) < n // 3
        if e < key_bits:
            assert (k["highbits"] >> e).max() > 0                       # bits at and above end_bit are set
    v = S.make_vals(n, 0)
    assert v.dtype == np.uint32 and len(np.unique(v)) > n // 2 and not np.array_equal(v, np.arange(n))


def test_depth_cases_yield_their_intended_control_words():
    for small in (False, True):
        tile = S.TILE_SMALL if small else S.TILE
        cases = {c.name.split("-", 1)[1]: c for c in S.depth_cases(small)}
        assert tuple(cases) == S.DEPTH_NAMES and all(c.small == small for c in cases.values())
        for bits in (8, 9, 16, 17, 24, 25, 32):
            c = cases["span%d" % bits]
            assert c.bits == bits and c.passes == (bits + 7) // 8 and c.base & 255 == 0 and c.n == 3 * tile + 5
            vis = c.keys != S.CULLED
            assert 0 < (~vis).sum() < c.n // 8
            lo, hi = c.keys[vis].min(), c.keys[vis].max()
            assert lo & 255 != 0 and c.base == int(lo) & ~255                     # the base is not simply the smallest key
            assert np.argmin(np.where(vis, c.keys, S.CULLED)) // tile == 3 and np.argmax(np.where(vis, c.keys, 0)) // tile == 0
            assert (c.keys == lo).sum() == 1 and (c.keys == hi).sum() == 1        # the extremes sit in those blocks only
            assert len(np.unique(c.keys)) < c.n // 3                              # ties
            assert c.nblk == 4 and c.nblk_pad == 16
        assert (cases["all-culled"].base, cases["all-culled"].bits, cases["all-culled"].passes) == (0, 8, 1)
        assert not (cases["all-culled"].keys != S.CULLED).any()
        c = cases["one-visible"]
        assert (c.keys != S.CULLED).sum() == 1 and (c.base, c.bits) == (0x40490FDB & ~255, 8) and c.nblk == 2
        c = cases["visible-equal"]
        assert len(np.unique(c.keys[c.keys != S.CULLED])) == 1 and c.bits == 8 and (c.keys == S.CULLED).any()
        c = cases["ninth-culled"]
        assert np.all(c.keys[::9] == S.CULLED) and (c.keys == S.CULLED).sum() == len(c.keys[::9]) and c.bits == 24
        c = cases["258-blocks"]
        assert c.n == 257 * tile + 1 and c.nblk == 258 and c.nblk_pad == 272 and c.bits == 24 and c.passes == 3
        vis = c.keys != S.CULLED
        assert np.argmin(np.where(vis, c.keys, S.CULLED)) // tile == 257          # read by the control workgroup's second lap only
        assert [b.passes for b in S.depth_batch(small)] == [1, 3, 4]
        assert len({b.n for b in S.depth_batch(small)}) == 1 and len({b.passes & 1 for b in S.depth_batch(small)}) == 2


def test_range_cases_hit_the_search_edges():
    assert S.RANGE_T == (1, 2, 254, 255, 256, 509, 510, 511, 8160) and S.RANGE_N == (0, 1, 4095, 4096, 4097, 8193, 100003)
    n_edges = 0
    for T in S.RANGE_T + (70000,):
        cases = S.range_cases(T)
        names = {c.name for c in cases}
        assert len(names) == len(cases)
        for n in S.RANGE_N:
            for lay in ("random", "tile0", "last_tile"):
                assert "T%d-n%d-%s" % (T, n, lay) in names
        assert "T%d-n%d-one_per_tile" % (T, T) in names
        for c in cases:
            assert c.keys.shape == (c.n,) and (c.n == 0 or c.keys.max() < T)
            if c.layout == "one_per_tile":
                assert np.array_equal(c.keys, np.arange(T))
            if c.layout == "gaps":
                r = S.ranges_reference(c.keys, c.n, T)
                empty = (r == 0).all(axis=1)
                assert empty[0] and empty[T - 1] and empty[T // 2] and not empty.all()    # front, middle, end
            if c.layout == "sample_edges":
                n_edges += 1
                js = {int(s) // S.RANGE_SAMPLE for s in c.run_starts if s % S.RANGE_SAMPLE == 0}
                assert js
                for j in js:
                    assert {S.RANGE_SAMPLE * j - 1, S.RANGE_SAMPLE * j, S.RANGE_SAMPLE * j + 1} <= set(int(s) for s in c.run_starts)
        if T >= 254:
            assert {"T%d-n%d-%s" % (T, n, lay) for n in (8193, 100003) for lay in ("gaps", "sample_edges")} <= names
    assert n_edges >= 2 * 8
    # the branches of the two-level search, by the reference's own numbers: a == 0 (tiles up to the first key), a == ns (tiles above
    # the last sample) and thread 255 closing the workgroup's last tile
    c = next(c for c in S.range_cases(8160) if c.name == "T8160-n100003-gaps")
    assert c.keys[0] > 0 and c.keys[-1] < T - 1 and c.keys[-1] > c.keys[(c.n - 1) // S.RANGE_SAMPLE * S.RANGE_SAMPLE]
    assert 8160 % S.RANGE_TILES_PER_WG == 0 and 510 % S.RANGE_TILES_PER_WG == 0 and 256 % S.RANGE_TILES_PER_WG == 1
    assert 8192 * 4096 // S.RANGE_SAMPLE == S.RANGE_MAX_SAMPLES and (8192 * 4096 + 1 + S.RANGE_SAMPLE - 1) // S.RANGE_SAMPLE > S.RANGE_MAX_SAMPLES


# ---- the checkers reject known-bad outputs ---------------------------------------------------------------------------------------
def _good_sort(c):
    keys, vals = S.case_arrays(c)
    ek, ev = S.sort_reference(keys, vals, c.end_bit)
    return keys, vals, ek.copy(), ev.copy()


@pytest.mark.parametrize("kind,given", [("u32", False), ("u32", True), ("u16", False), ("small", False)])
def test_sort_checker_accepts_the_reference_and_rejects_bad_outputs(kind, given):
    c = S.sort_case(kind, 10007, S.SIZE_END_BIT[kind], "ties", given)
    keys, vals, ek, ev = _good_sort(c)
    S.check_sort(keys, vals, c.end_bit, ek, ev)
    mask = (1 << c.end_bit) - 1
    i = int(np.nonzero((ek[1:] & mask) == (ek[:-1] & mask))[0][0])       # two tied neighbours swapped: keys still sorted
    bk, bv = ek.copy(), ev.copy()
    bk[[i, i + 1]], bv[[i, i + 1]] = bk[[i + 1, i]], bv[[i + 1, i]]
    assert np.array_equal(bk & mask, ek & mask) and not np.array_equal(bv, ev)
    with pytest.raises(AssertionError):
        S.check_sort(keys, vals, c.end_bit, bk, bv)
    bk, bv = ek.copy(), ev.copy()                                        # one element duplicated over another
    bk[i + 1], bv[i + 1] = bk[i], bv[i]
    with pytest.raises(AssertionError):
        S.check_sort(keys, vals, c.end_bit, bk, bv)


def test_sort_checker_wants_the_ignored_key_bits_back():
    c = S.sort_case("u32", 4097, 13, "highbits", False)
    keys, vals, ek, ev = _good_sort(c)
    assert (ek >> 13).max() > 0
    S.check_sort(keys, vals, 13, ek, ev)
    with pytest.raises(AssertionError):
        S.check_sort(keys, vals, 13, ek & 0x1FFF, ev)        # sorted bits right, upper bits lost
    full_order = np.argsort(keys, kind="stable")              # sorted on all 32 bits: the upper bits were not ignored
    with pytest.raises(AssertionError):
        S.check_sort(keys, vals, 13, keys[full_order], full_order.astype(np.uint32))


def _good_depth(c):
    """a valid output: visible entries in stable order, culled ones scattered among them as their low bits would have it"""
    base, bits, passes = S.expected_ctl(c.keys)
    m = np.uint32((1 << (8 * passes)) - 1) if passes < 4 else np.uint32(0xFFFFFFFF)
    order = np.argsort((c.keys - np.uint32(base)) & m, kind="stable").astype(np.uint32)
    return c.keys[order], order, np.array([base, bits, passes, 0], dtype=np.int64)


def test_depth_checker_accepts_valid_outputs_and_rejects_bad_ones():
    for c in S.depth_cases(True)[:7] + S.depth_cases(False)[7:11]:
        ko, vo, ctl = _good_depth(c)
        S.check_depth(c.keys, ko, vo, ctl)
        S.check_depth(c.keys, ko, vo, ctl.astype(np.uint32).view(np.int32))  # (the probe's words arrive as signed integers)
        vis = np.nonzero(ko != S.CULLED)[0]
        if vis.size == 0:
            continue
        for delta in (8, -8):                                                # a control word off by one pass
            bad = ctl.copy()
            bad[1] = ctl[1] + delta
            bad[2] = S.depth_sort_passes(int(bad[1]))
            if 8 <= bad[1] <= 32:
                with pytest.raises(AssertionError):
                    S.check_depth(c.keys, ko, vo, bad)
        bad = ctl.copy()
        bad[2] += 1
        with pytest.raises(AssertionError):
            S.check_depth(c.keys, ko, vo, bad)
        bad = ctl.copy()
        bad[0] += 256
        with pytest.raises(AssertionError):
            S.check_depth(c.keys, ko, vo, bad)
        if vis.size >= 2:
            tied = [int(p) for p, q in zip(vis[:-1], vis[1:]) if ko[p] == ko[q]]
            if tied:                                                         # two tied visible entries swapped
                p = tied[0]
                q = int(vis[np.searchsorted(vis, p) + 1])
                bk, bv = ko.copy(), vo.copy()
                bk[[p, q]], bv[[p, q]] = bk[[q, p]], bv[[q, p]]
                with pytest.raises(AssertionError):
                    S.check_depth(c.keys, bk, bv, ctl)
            p, q = int(vis[0]), int(vis[-1])                                 # one element duplicated over another
            bk, bv = ko.copy(), vo.copy()
            bk[q], bv[q] = bk[p], bv[p]
            with pytest.raises(AssertionError):
                S.check_depth(c.keys, bk, bv, ctl)
        bk = ko.copy()                                                       # a key that lost its value
        bk[int(vis[0])] ^= 1
        with pytest.raises(AssertionError):
            S.check_depth(c.keys, bk, vo, ctl)
    # where the culled entries land is not asserted: all of them at the end is as good as anything
    c = S.depth_cases(True)[4]
    order = np.argsort(c.keys, kind="stable").astype(np.uint32)
    S.check_depth(c.keys, c.keys[order], order, np.array([c.base, c.bits, c.passes, 0], dtype=np.uint32))


def test_ranges_checker_rejects_bad_ranges():
    c = next(c for c in S.range_cases(511) if c.name == "T511-n8193-gaps")
    good = S.ranges_reference(c.keys, c.n, c.T)
    S.check_ranges(c.keys, c.n, c.T, good)
    S.check_ranges(c.keys, c.n, c.T, good.astype(np.int32))
    assert good[c.keys[0]][0] == 0 and good[c.keys[-1]][1] == c.n
    t = c.T // 2                                                             # an empty tile of the middle gap
    k = int(np.searchsorted(c.keys, t))
    assert (good[t] == 0).all() and 0 < k < c.n
    bad = good.copy()
    bad[t] = (k, k)                                                          # an empty tile as (k, k) instead of (0, 0)
    with pytest.raises(AssertionError):
        S.check_ranges(c.keys, c.n, c.T, bad)
    t = int(c.keys[c.n // 2])
    for col, d in ((0, 1), (0, -1), (1, 1), (1, -1)):                        # a bound off by one
        bad = good.copy()
        bad[t, col] += d
        with pytest.raises(AssertionError):
            S.check_ranges(c.keys, c.n, c.T, bad)
    bad = good.copy()
    bad[0] = -1                                                              # a tile the kernel never wrote (the probe's fill)
    with pytest.raises(AssertionError):
        S.check_ranges(c.keys, c.n, c.T, bad.astype(np.int32))
    # counts: only the first n keys count
    r = S.ranges_reference(c.keys, 1, c.T)
    assert r[c.keys[0]].tolist() == [0, 1] and (r != 0).sum() == 1
    assert (S.ranges_reference(c.keys, 0, c.T) == 0).all()
