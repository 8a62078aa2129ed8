"""The batched sweep's case generator (tests/batch_cases.py) without a GPU: the census of the launch branches its default range
reaches, its determinism, its launch formulas against hand-computed values, and the reference-only check -- on these inputs the
reference ARITHMETIC alone (the plain-C oracle's float32 restatement, summed over the views) must stay within the caps that
tests/test_gpu_batch_fuzz.py applies to the library's `reference_outside_too` rows, measured against float64."""
import numpy as np

import batch_cases as BC
import util
from grad_ladder import MAX_CASE_FRACTION_REF_TOO, MAX_ROW_FRACTION_REF_TOO, Float64

SMALL = list(range(BC.N_SMALL))
REF_ONLY = SMALL           # the reference-only check runs the whole small class (under a minute on 16 CPUs)


def test_launch_formulas_at_known_shapes():
    # preprocess.hip: the benchmark's shapes (12 views of 200 K / 800 K points) and the ragged rows of the issue
    assert BC.preprocess_vpt(12, 200_000) == (4, 3, 4)
    assert BC.preprocess_vpt(12, 800_000) == (12, 1, 12)
    assert BC.preprocess_vpt(12, 12_000) == (1, 12, 1)
    assert BC.preprocess_vpt(5, 300_000) == (4, 2, 1)
    assert BC.preprocess_vpt(12, 300_000) == (8, 2, 4)
    assert BC.preprocess_vpt(12, 100_000) == (2, 6, 2)
    assert BC.preprocess_vpt(3, 530_000) == (3, 1, 3)
    assert BC.preprocess_vpt(7, 180_000) == (2, 4, 1)
    assert BC.preprocess_vpt(1, 5_000_000) == (1, 1, 1)
    # render_bwd.hip: 12 x 1080p pulls its units, 3 x 208x176 does not, 256 x 256x144 does by view count alone
    assert BC.backward_dynamic(12, 120 * 68) and not BC.backward_dynamic(3, 13 * 11) and BC.backward_dynamic(256, 16 * 9)
    assert not BC.backward_dynamic(1, 240 * 135)
    assert [BC.tile_sort_passes(T) for T in (1, 91, 255, 256, 704, 65535, 65536)] == [1, 1, 1, 2, 2, 2, 3]
    assert (BC.slice_length(1), BC.slice_length(2), BC.slice_length(256)) == (512, 1024, 1024)
    k = np.float32([2.0]).view(np.uint32)[0]
    assert BC.depth_sort_words([]) == (0, 8, 1)
    assert BC.depth_sort_words([k, k + 255]) == (int(k), 8, 1)
    assert BC.depth_sort_words([k + 3, k + 256]) == (int(k), 9, 2)
    assert BC.depth_sort_words([k, k + 0xFFFF])[1:] == (16, 2) and BC.depth_sort_words([k, k + 0x10000])[1:] == (17, 3)
    assert BC.depth_sort_words(np.float32([0.25, 60.0]).view(np.uint32))[2] == 4


def test_tile_sort_passes_follow_the_oracle_s_msb(oracle):
    for T in (1, 2, 91, 255, 256, 257, 475, 704, 8160):
        assert BC.tile_sort_passes(T) == (oracle.get_higher_msb(T) + 7) // 8, T


def test_generator_is_deterministic():
    for i in (0, 3, 17, 40, 95, BC.MEDIUM_BASE + 6):
        a, b = BC.case(i), BC.case(i)
        assert BC.fingerprint(a) == BC.fingerprint(b), i
        assert BC.dL_dpix(a).tobytes() == BC.dL_dpix(b).tobytes()
        assert BC.expected(i, a) == BC.expected(i, b)
    assert BC.fingerprint(BC.case(1)) != BC.fingerprint(BC.case(2))


def test_cases_are_valid_batches():
    for i in BC.ids():
        if i >= BC.MEDIUM_BASE + 1:
            continue                                   # (the medium clouds are built alike: one is enough here)
        c = BC.case(i)
        V = len(c["views"])
        assert 2 <= V <= BC.MAX_VIEWS
        assert len({(v["tanfovx"], v["tanfovy"]) for v in c["views"]}) == 1, "a batch shares its field of view"
        assert all(0 <= v < V for v in c["empty"])
        assert all(np.isfinite(v[k]).all() for v in c["views"] for k in ("viewmatrix", "projmatrix", "campos"))
        s = BC.scenes(c)
        assert len(s) == V and s[0].P == c["g"]["means3D"].shape[0] and (s[0].W, s[0].H) == (c["W"], c["H"])


def census(ids):
    exp = [BC.expected(i) for i in ids if i < BC.MEDIUM_BASE]
    # (the medium cases: the formulas only, without building their clouds)
    for j, (V, P, W, H) in enumerate(BC.MEDIUM):
        if BC.MEDIUM_BASE + j in ids:
            T = ((W + 15) // 16) * ((H + 15) // 16)
            vpt, rows, last = BC.preprocess_vpt(V, P)
            exp.append(dict(V=V, P=P, W=W, H=H, T=T, vpt=vpt, grid_rows=rows, last_row_views=last, ragged=last != vpt,
                            dynamic=BC.backward_dynamic(V, T), tile_sort_passes=BC.tile_sort_passes(T), empty=[], mixed=False,
                            depth_passes=None))
    return exp


def test_census_of_the_default_range():
    exp = census(BC.ids())
    vpts = {e["vpt"] for e in exp}
    assert {1, 2, 4, 8} <= vpts, vpts
    assert any(e["vpt"] == e["V"] and e["grid_rows"] == 1 and e["V"] > 1 for e in exp)
    assert sum(e["ragged"] for e in exp) >= 2
    assert any(e["dynamic"] for e in exp) and any(not e["dynamic"] for e in exp)
    assert any(e["dynamic"] and e["T"] <= 256 for e in exp), "no small image takes the pulled units by view count alone"
    assert {e["tile_sort_passes"] for e in exp} >= {1, 2}
    assert any(256 < e["T"] <= 704 for e in exp) and any(e["T"] <= 255 for e in exp)
    assert any(e["V"] == 256 for e in exp)
    assert any(0 in e["empty"] for e in exp), "no empty first view"
    assert any(e["V"] - 1 in e["empty"] for e in exp), "no empty last view"
    assert any(any(0 < v < e["V"] - 1 for v in e["empty"]) for e in exp), "no empty middle view"
    mixed = [e for e in exp if e["mixed"]]
    assert len(mixed) >= 3, len(mixed)
    # every pass count is predicted somewhere, and a mixed batch holds odd and even counts (the emission reads buffer passes & 1)
    assert {p for e in mixed for p in e["depth_passes"] if p is not None} == {1, 2, 3, 4}
    print("census: V %s, vpt %s, ragged %d, dynamic %d, two tile-sort passes %d, empty views in %d cases, mixed pass counts in %d" % (
        sorted({e["V"] for e in exp}), sorted(vpts), sum(e["ragged"] for e in exp), sum(e["dynamic"] for e in exp),
        sum(e["tile_sort_passes"] == 2 for e in exp), sum(bool(e["empty"]) for e in exp), len(mixed)))


def test_slab_views_are_predicted_as_built():
    """where the host can tell, a slab view needs the pass count it was built for"""
    told = 0
    for i in SMALL:
        c = BC.case(i)
        if not c["slab"]:
            continue
        e = BC.expected(i, c)
        for want, got in zip(c["want_passes"], e["depth_passes"]):
            if got is not None:
                assert got == want, (i, c["want_passes"], e["depth_passes"])
                told += 1
    assert told >= 20, told


def reference_only_shares(ids, nthreads=16):
    """(cases, cases with a row outside, rows, rows outside, per-case lines): the oracle's float32 restatement summed over the
    views against float64 summed over the views, at the plain row bar"""
    cases = bad_cases = rows = bad_rows = 0
    lines = []
    for i in ids:
        c = BC.case(i)
        f64 = Float64(BC.scenes(c), BC.dL_dpix(c), nthreads=nthreads)
        tot = f64.total()
        cases += 1
        n_bad = 0
        for k in util.GRAD_NAMES:
            b = np.asarray(tot[k], np.float64)
            if b.size == 0:
                continue
            a = sum(np.asarray(w["grads32"][k], np.float64).reshape(b.shape) for w in f64.views())
            a2, b2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
            rn = np.linalg.norm(b2, axis=1)
            out = np.linalg.norm(a2 - b2, axis=1) > util.ROW_REL * rn + util.ROW_ABS * rn.max() + 1e-30
            rows += int(a.shape[0])
            n_bad += int(out.sum())
        if n_bad:
            bad_cases += 1
            lines.append("case %d (V=%d P=%d %dx%d): %d rows outside" % (i, len(c["views"]), c["g"]["means3D"].shape[0], c["W"], c["H"], n_bad))
        bad_rows += n_bad
    return cases, bad_cases, rows, bad_rows, lines


def test_reference_arithmetic_alone_meets_the_caps(oracle):
    cases, bad_cases, rows, bad_rows, lines = reference_only_shares(REF_ONLY)
    print("reference-only check over %d cases: %d cases / %d of %d rows outside the plain row bar against float64 (%.3g / %.3g)" % (
        cases, bad_cases, bad_rows, rows, bad_cases / cases, bad_rows / max(rows, 1)))
    for ln in lines:
        print("  " + ln)
    # the caps as tests/test_gpu_fuzz.py applies them (its floors of 2 cases / 8 rows included)
    assert bad_cases <= max(2, int(MAX_CASE_FRACTION_REF_TOO * cases)), (bad_cases, cases, lines)
    assert bad_rows <= max(8, int(MAX_ROW_FRACTION_REF_TOO * rows)), (bad_rows, rows, lines)
