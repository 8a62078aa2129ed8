"""The gradient comparison of the randomised sweeps (tests/test_gpu_fuzz.py: one view; tests/test_gpu_batch_fuzz.py: sums over the
views of a batch; tests/test_gpu_channel_fuzz.py: the same with the extra channels' share, ChannelsFloat64), with its fallbacks
counted.

A library gradient tensor is first held to the reference build's by util.grad_violations.  On a violation the ladder is
  1. float64, summed over the views, is the arbiter: the oracle's float64 render backward per view feeding the float64 chain of
     tests/fp64_backward.py;
  2. the plain row bar (util.ROW_REL, util.ROW_ABS) against it;
  3. 4 x the reference build's own distance from it, row by row;
  4. the conditioning exit: noise of the size of float32 rounding pushed through the float64 chain per view, and the float32 chain.
Every exit is tallied (new_tally); the sweeps cap the tallies."""
import numpy as np

import util
from fp64_backward import gaussian_backward_fp64

RENDER = ("dL_dmean2D", "dL_dconic", "dL_dcolor")


def new_tally():
    return dict(cases=0, rows=0, cases_exit_4x_reference=0, rows_exit_4x_reference=0, cases_exit_conditioning=0, rows_exit_conditioning=0,
                cases_reference_outside_too=0, rows_reference_outside_too=0)


class Float64:
    """The float64 gradients of a batch of views of one cloud, computed when first asked for.
    views(): per view dict(fwd = the oracle's forward, exact = float64 render-level sums, f32 = the double sums of the oracle's
    float32 terms, grads32 = the oracle's float32 restatement); total(): the eight gradients summed over the views."""

    def __init__(self, scenes, dLs, nthreads=1):
        self.scenes, self.dLs, self.nthreads = scenes, dLs, nthreads
        self._views = self._total = None

    def views(self):
        if self._views is None:
            from oracle.oracle import Oracle
            orc = Oracle()
            kw = {} if self.nthreads == 1 else dict(nthreads=self.nthreads)
            self._views = []
            for s, dL in zip(self.scenes, self.dLs):
                of, og = orc.forward_backward(s, dL, exact=True, **kw)
                self._views.append(dict(fwd=of, exact=og["exact"], f32={n: og[n] for n in RENDER}, grads32=og))
        return self._views

    def chain(self, v, sums, rows=None, dtype=np.float64):
        w = self.views()[v]
        return gaussian_backward_fp64(self.scenes[v], w["fwd"]["radii"], w["fwd"]["clamped"], sums["dL_dmean2D"], sums["dL_dconic"],
                                      sums["dL_dcolor"], rows=rows, dtype=dtype)

    def total(self):
        if self._total is None:
            tot = {}
            for v, w in enumerate(self.views()):
                og = dict(w["grads32"], **w["exact"])      # render-level sums: the float64 ones
                og.update(self.chain(v, w["exact"]))
                for k, a in og.items():
                    if k != "exact":
                        tot[k] = tot.get(k, 0.0) + np.asarray(a, np.float64)
            self._total = tot
        return self._total


class ChannelsFloat64(Float64):
    """Float64 for a channels backward: the render-level sums of a view are those of its colour run plus one colors_precomp run per
    group of three extra channels (tests/fp64_channels.channels_backward_fp64_scenes, computed when first asked for); the chain is
    linear in them, so chain() and the noise model of hold_to_reference apply unchanged.  result(): that function's dict (per view
    also opacity, colour and extra, the records and dL/d values of the view)."""

    def __init__(self, scenes, dense_extra, scale, bg_extra, dLs, dL_dextra, nthreads=1):
        Float64.__init__(self, scenes, dLs, nthreads)
        self.extra = (dense_extra, scale, bg_extra, dL_dextra)
        self._result = None

    def result(self):
        if self._result is None:
            from fp64_channels import channels_backward_fp64_scenes
            from oracle.oracle import Oracle
            dense, scale, bgx, dx = self.extra
            self._result = channels_backward_fp64_scenes(Oracle(), self.scenes, dense, scale, bgx, self.dLs, dx, nthreads=self.nthreads)
        return self._result

    def views(self):
        if self._views is None:
            self._views = self.result()["views"]
        return self._views

    def total(self):
        return self.result()["grads"]


def hold_to_reference(tag, seed, gp, gr, f64, tally, label="fuzz"):
    """gp: the library's gradients (summed over the views), gr: the reference build's (summed likewise), f64: a Float64 of the same
    views and image gradients.  Asserts the ladder of the module docstring and counts its exits in `tally`."""
    tally["cases"] += 1
    used_4x = used_cond = used_ref_too = False
    V = len(f64.scenes)
    for k, a in gp.items():
        b = gr[k]
        if a.size == 0 and b.size == 0:
            continue
        assert a.shape == b.shape, "%s %s" % (tag, k)
        assert np.isfinite(a).all(), "%s %s" % (tag, k)
        tally["rows"] += int(a.shape[0])
        scale = np.abs(b).max()
        d_ref = np.abs(a.astype(np.float64) - b.astype(np.float64)).max()
        bad_el, bad_row, _ = util.grad_violations(a, b)
        if bad_el == 0 and bad_row == 0:
            continue
        # Both sides sum thousands of fp32 terms in different (for the reference: unspecified, atomic) orders, and the
        # per-Gaussian chain conic -> cov3D -> scale / rotation / mean can amplify that rounding noise by 10^3..10^5 on an
        # ill-conditioned splat (a nearly singular conic).  The plain-C oracle's float32 restatement is no arbiter there: it
        # evaluates every per-(pixel, entry) term and that chain in float32 with the reference's own expression order, so it
        # shares the reference build's rounding (the double SUMS of those float32 terms lie 2e-7..8e-7 of max|g| from the
        # true sums on the parity scenes, more than either implementation's summation error).  The exact value comes from
        # float64 end to end: the oracle's float64 render backward (orc_render_backward_fp64: every term in double, the
        # float forward's hit / stop decisions) feeding the float64 chain of tests/fp64_backward.py; the library must be
        # inside the usual bar against it, or no further from it than 4x the reference build's own distance, row by row.
        o = np.asarray(f64.total()[k], np.float64).reshape(a.shape[0], -1)
        a2, b2 = a.astype(np.float64).reshape(a.shape[0], -1), b.astype(np.float64).reshape(a.shape[0], -1)
        rn = np.linalg.norm(o, axis=1)
        r_lib, r_build = np.linalg.norm(a2 - o, axis=1), np.linalg.norm(b2 - o, axis=1)
        plain = r_lib <= util.ROW_REL * rn + util.ROW_ABS * rn.max() + 1e-30          # the usual row bar, against the exact value
        ok = r_lib <= np.maximum(util.ROW_REL * rn + util.ROW_ABS * rn.max(), 4 * r_build) + 1e-30
        no_worse = ~plain & (r_lib <= r_build)          # the reference build is outside the bar too, and further out
        if no_worse.any():
            used_ref_too = True
            tally["rows_reference_outside_too"] += int(no_worse.sum())
        n4 = int((ok & ~plain & ~no_worse).sum())
        if n4:
            used_4x = True
            tally["rows_exit_4x_reference"] += n4
            w = np.nonzero(ok & ~plain & ~no_worse)[0]
            print("%s exit (4x reference): %s %s rows %s: lib-exact %s, ref-exact %s, row bar %s" % (
                label, tag, k, w.tolist()[:4], r_lib[w][:4], r_build[w][:4], (util.ROW_REL * rn + util.ROW_ABS * rn.max())[w][:4]))
        if not ok.all() and k in ("dL_dmean3D", "dL_dcov3D", "dL_dscale", "dL_drot"):
            # Still outside: is the row simply that ill-conditioned?  (a) The render-level sums every float32 implementation
            # feeds into the chain carry rounding noise: push noise of that size through the float64 chain and see how far the
            # exact result moves.  (b) The chain itself rounds: run the very same expressions in float32 and see how far THAT
            # lands from the float64 result.  A row passes if the library is within 6 sigma of (a) or within 4x the distance
            # (b) -- i.e. as good as float32 arithmetic gets on that splat.  (A batch: per view, the results summed.)
            bad = np.nonzero(~ok)[0]
            rng = np.random.default_rng(seed)
            views = f64.views()
            base = sum(f64.chain(v, views[v]["exact"], rows=bad)[k] for v in range(V))
            dev = np.zeros(bad.size)
            for _ in range(8):
                # size of the noise, per element: relative 1e-6, plus an absolute floor of 2e-7 of the array's largest entry (a
                # per-Gaussian sum over pixels of terms of both signs can cancel, its rounding noise does not shrink with it: two
                # runs of this library differ by that much in dL_dmean2D -- float atomics commit in arrival order --
                # scripts/diag_fuzz_state.py), plus the distance between the float32 per-(pixel, entry) terms (the reference's
                # arithmetic, summed without error: the oracle's float32 restatement) and the float64 value of the same sum --
                # what evaluating power / exp / the recurrences in float32 costs on THIS splat whatever the summation (a needle
                # 100 pixels long seen from half a unit away: 7e-5 of the value, where a compact splat has 1e-7)
                out = 0.0
                for v in range(V):
                    og = views[v]["exact"]
                    f32 = {n: np.asarray(views[v]["f32"][n], np.float64).reshape(np.asarray(og[n]).shape) for n in RENDER}
                    noisy = {n: np.asarray(og[n], np.float64) * (1.0 + 1e-6 * rng.standard_normal(np.asarray(og[n]).shape))
                             + 2e-7 * np.abs(np.asarray(og[n], np.float64)).max() * rng.standard_normal(np.asarray(og[n]).shape)
                             + np.abs(f32[n] - np.asarray(og[n], np.float64)) * rng.standard_normal(np.asarray(og[n]).shape)
                             for n in RENDER}
                    out = out + f64.chain(v, noisy, rows=bad)[k]
                dev += ((out - base).reshape(bad.size, -1) ** 2).sum(1)
            sigma = np.sqrt(dev / 8)
            c32 = sum(f64.chain(v, views[v]["exact"], rows=bad, dtype=np.float32)[k].astype(np.float64) for v in range(V))
            r_f32 = np.sqrt(((c32 - base).reshape(bad.size, -1) ** 2).sum(1))
            ok[bad] = r_lib[bad] <= np.maximum(6 * sigma, 4 * r_f32)
            if ok[bad].any():
                used_cond = True
                tally["rows_exit_conditioning"] += int(ok[bad].sum())
                # how large the float32-vs-float64 term of the noise model is when this exit fires (relative to the exact sums): a
                # drift of this term -- the exit leaning on it more and more -- shows here
                f32_term = max(float(np.abs(np.asarray(w["f32"][n], np.float64).reshape(np.asarray(w["exact"][n]).shape)
                                            - np.asarray(w["exact"][n], np.float64)).max()
                                     / (np.abs(np.asarray(w["exact"][n], np.float64)).max() + 1e-300)) for n in RENDER for w in views)
                tally["max_f32_term_at_conditioning_exit"] = max(tally.get("max_f32_term_at_conditioning_exit", 0.0), f32_term)
                print("%s exit (conditioning): %s %s rows %s: lib-exact %s, 6 sigma %s, 4 x f32 chain %s; |f32 terms - f64| up to %.2e of max|g|"
                      % (label, tag, k, bad[ok[bad]].tolist()[:4], r_lib[bad][ok[bad]][:4], (6 * sigma)[ok[bad]][:4], (4 * r_f32)[ok[bad]][:4],
                         f32_term))
        assert ok.all(), "%s %s: %d rows; worst lib-exact %.3g (ref-exact %.3g there), lib-ref max %.3g, max|g| %.3g" % (
            tag, k, int((~ok).sum()), r_lib[~ok].max(), r_build[~ok][np.argmax(r_lib[~ok])], d_ref, scale)
    tally["cases_exit_4x_reference"] += int(used_4x)
    tally["cases_exit_conditioning"] += int(used_cond)
    tally["cases_reference_outside_too"] += int(used_ref_too and not (used_4x or used_cond))


# How often a case / a gradient row may leave through a fallback of hold_to_reference.  The bars are principled (float32 conditioning
# of the per-Gaussian chain), but nothing stops them from being widened until everything passes, so the exits are counted and capped:
# the closing test of every sweep fails when more than 1 % of the cases or 1e-4 of the rows compared need one.
# `*_reference_outside_too`: rows outside the plain bar against the float64 value in which the library is at least as close to it as
# the reference build is -- the reference itself misses the bar there; not an escape of the library, but a drift towards such rows
# should still show: a looser cap of its own
MAX_CASE_FRACTION = 0.01
MAX_ROW_FRACTION = 1e-4
MAX_CASE_FRACTION_REF_TOO = 0.02
MAX_ROW_FRACTION_REF_TOO = 4e-4


def assert_exits_stay_rare(tally, max_case_fraction, max_row_fraction, max_case_fraction_ref_too, max_row_fraction_ref_too):
    cases = tally["cases_exit_4x_reference"] + tally["cases_exit_conditioning"]
    rows = tally["rows_exit_4x_reference"] + tally["rows_exit_conditioning"]
    # (at least one case is always allowed: small sweeps must not fail on a single ill-conditioned splat)
    assert cases <= max(1, int(max_case_fraction * tally["cases"])), tally
    assert rows <= max(2, int(max_row_fraction * tally["rows"])), tally
    assert tally["cases_reference_outside_too"] <= max(2, int(max_case_fraction_ref_too * tally["cases"])), tally
    assert tally["rows_reference_outside_too"] <= max(8, int(max_row_fraction_ref_too * tally["rows"])), tally
    # the float32-evaluation term of the conditioning exit's noise model stays what it was introduced for (needles: ~7e-5)
    assert tally.get("max_f32_term_at_conditioning_exit", 0.0) <= 1e-3, tally
