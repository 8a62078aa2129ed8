// footprint_bound_main.cpp -- stand-alone host check of the footprint test's algebra (csrc/tile_cull.hpp: may_touch_rect).
// Built and run by tests/test_cpu_footprint_bound.py:
//     hipcc --cuda-host-only -O2 -ffp-contract=off -I gaussian-pcloud-render_amd/csrc tests/footprint_bound_main.cpp -o footprint_bound
//     ./footprint_bound [cases = 1048576] [seed = 1]
// (also fit for -fsanitize=address,undefined: it is an ordinary host program).  It prints one line of JSON.
//
// Seeded random (conic, centre, rectangle, opacity) cases:
//   rectangles  w x h pixels, 1 <= w, h <= 8, a quarter of them forced to one pixel, one row or one column;
//   centres     in each of the nine regions around the rectangle (inside, beside the four edges, diagonal to the four corners),
//               0.01 .. 40 pixels beyond the edge;
//   conics      inverted in float32 from sigma_1, sigma_2 in [0.3, 30] pixels and a correlation rho, |rho| up to 0.999 (half of the
//               cases with 1 - |rho| log-uniform in [1e-3, 1]);
//   opacities   a third around 1/255, a third placed so that the rectangle's best pixel sits within +-0.2 % of the alpha = 1/255
//               threshold (the cases in which a non-conservative bound would show), the rest uniform in (0, 1].
// Checked:
//   (a) misses: cases in which some pixel centre of the rectangle counts under the kernels' own float32 rule
//       (!(power > 0) && !(min(0.99, o exp(power)) < 1/255)) and may_touch_rect says "provably not".  Must be 0.
//   (b) the cases may_touch_rect keeps and the four-edge form it replaced (kept below as may_touch_rect_4edge) drops: the
//       price of leaving the far edges and the full-precision logarithm out, as a count.
//   (c) NaN in any of the six splat inputs keeps.
// The device's v_rcp_f32 / v_log_f32 are not exercised here (the host build takes 1/x and log2f): the GPU tests cover them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "tile_cull.hpp"

// the form this test replaced: centre inside -> 0, else the maximum over all four edges; threshold from the full logf
static bool may_touch_rect_4edge(float mx, float my, float A, float B, float C, float o, float x0, float y0, float x1, float y1)
{
    if (o <= 0.f) return false;
    if (!(A > 0.f && C > 0.f && A * C - B * B > 0.f)) return true;
    const float thr = -logf(255.0f * o);
    const float dxl = mx - x1, dxh = mx - x0, dyl = my - y1, dyh = my - y0;
    float m;
    if (dxl <= 0.f && dxh >= 0.f && dyl <= 0.f && dyh >= 0.f) {
        m = 0.f;
    } else {
        m = -3.0e38f;
        const float nB_over_C = -B * (1.0f / C), nB_over_A = -B * (1.0f / A);
        for (int e = 0; e < 2; e++) {
            const float ex = e ? dxh : dxl;
            const float yy = gsr::clampf(nB_over_C * ex, dyl, dyh);
            m = fmaxf(m, -0.5f * (A * ex * ex + C * yy * yy) - B * ex * yy);
            const float ey = e ? dyh : dyl;
            const float xx = gsr::clampf(nB_over_A * ey, dxl, dxh);
            m = fmaxf(m, -0.5f * (A * xx * xx + C * ey * ey) - B * xx * ey);
        }
    }
    const float ax = fmaxf(fabsf(dxl), fabsf(dxh)), ay = fmaxf(fabsf(dyl), fabsf(dyh));
    const float E = 1.0e-5f * (A * ax * ax + C * ay * ay + fabsf(B) * ax * ay) + 1.0e-4f + 1.0e-5f * fabsf(thr);
    return !(m + E < thr);
}

// the kernels' per-pixel rule (render_fwd.hip eval_pair), one pixel; best = the largest float32 power seen over the rectangle
static bool pixel_counts(float mx, float my, float A, float B, float C, float o, float px, float py, float& best)
{
    const float dx = mx - px, dy = my - py;
    const float power = -0.5f * (A * dx * dx + C * dy * dy) - B * dx * dy;
    if (power > best) best = power;
    const float alpha = fminf(0.99f, o * expf(power));
    return !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
}

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }          // [0, 1)
    double uni(double a, double b) { return a + (b - a) * uni(); }
    double logu(double a, double b) { return a * std::exp(std::log(b / a) * uni()); }     // log-uniform in [a, b)
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

int main(int argc, char** argv)
{
    const long cases = argc > 1 ? atol(argv[1]) : 1l << 20;
    Rng r{argc > 2 ? (uint64_t)atoll(argv[2]) : 1ull};
    long misses = 0, counted = 0, kept_new = 0, kept_old = 0, new_not_old = 0, old_not_new = 0;
    long region_n[9] = {0}, rho_999 = 0, one_px = 0, one_row = 0, one_col = 0, near_255 = 0, razor = 0;
    for (long c = 0; c < cases; c++) {
        // rectangle
        uint32_t w = 1 + r.below(8), h = 1 + r.below(8);
        switch (r.below(12)) { case 0: w = h = 1; break; case 1: h = 1; break; case 2: w = 1; break; default: break; }
        one_px += w == 1 && h == 1; one_row += h == 1 && w > 1; one_col += w == 1 && h > 1;
        const float x0 = (float)r.below(1913), y0 = (float)r.below(1073), x1 = x0 + (float)(w - 1), y1 = y0 + (float)(h - 1);
        // centre: region (rx, ry) in {0 below, 1 within, 2 above} per axis
        const uint32_t reg = (uint32_t)(c % 9), rx = reg % 3, ry = reg / 3;
        region_n[reg]++;
        const float mx = rx == 1 ? (float)r.uni(x0, x1 == x0 ? x0 : x1) : rx == 0 ? x0 - (float)r.logu(0.01, 40.) : x1 + (float)r.logu(0.01, 40.);
        const float my = ry == 1 ? (float)r.uni(y0, y1 == y0 ? y0 : y1) : ry == 0 ? y0 - (float)r.logu(0.01, 40.) : y1 + (float)r.logu(0.01, 40.);
        // conic = inverse of the 2 x 2 covariance, in float32 like the preprocess
        const float s1 = (float)r.logu(0.3, 30.), s2 = (float)r.logu(0.3, 30.);
        float rho = (r.next() & 1) ? (float)(1.0 - r.logu(1e-3, 1.0)) : (float)r.uni(0., 0.9);
        if (r.next() & 1) rho = -rho;
        rho_999 += fabsf(rho) > 0.99f;
        const float sxx = s1 * s1, syy = s2 * s2, sxy = rho * s1 * s2;
        const float det = sxx * syy - sxy * sxy;
        if (!(det > 0.f)) { c--; region_n[reg]--; continue; }
        const float A = syy / det, B = -sxy / det, C = sxx / det;
        // opacity
        float o;
        const uint32_t okind = r.below(3);
        if (okind == 0) {
            o = (1.0f / 255.0f) * (float)r.uni(0.9, 1.5);
            near_255++;
        } else if (okind == 1) {
            // the best pixel's alpha within +-0.2 % of 1/255: o = exp(-best) / 255 * (1 + delta)
            float best = -3.0e38f;
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++) pixel_counts(mx, my, A, B, C, 1.f, x0 + (float)x, y0 + (float)y, best);
            const double oo = std::exp(-(double)best) / 255.0 * (1.0 + r.uni(-2e-3, 2e-3));
            if (oo <= 1.0) { o = (float)oo; razor++; } else o = (float)r.uni(1e-3, 1.0);
        } else {
            o = (float)r.uni(1e-3, 1.0);
        }
        // (a)
        bool any = false;
        float best = -3.0e38f;
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) any = pixel_counts(mx, my, A, B, C, o, x0 + (float)x, y0 + (float)y, best) || any;
        const bool kn = gsr::may_touch_rect(mx, my, A, B, C, o, x0, y0, x1, y1);
        const bool ko = may_touch_rect_4edge(mx, my, A, B, C, o, x0, y0, x1, y1);
        counted += any;
        if (any && !kn) {
            if (misses < 5)
                fprintf(stderr, "miss: mean %.9g %.9g conic %.9g %.9g %.9g o %.9g rect %g %g %g %g\n", mx, my, A, B, C, o, x0, y0, x1, y1);
            misses++;
        }
        kept_new += kn; kept_old += ko;
        new_not_old += kn && !ko;
        old_not_new += ko && !kn;
    }
    // (c) NaN in any input keeps
    const float nan = std::numeric_limits<float>::quiet_NaN();
    int nan_drops = 0;
    for (int i = 0; i < 6; i++) {
        float v[6] = {100.f, 50.f, 0.5f, 0.1f, 0.4f, 0.001f};   // (a splat 90 pixels from the rectangle at opacity 0.001: dropped as it is)
        const bool base = gsr::may_touch_rect(v[0], v[1], v[2], v[3], v[4], v[5], 8.f, 8.f, 15.f, 15.f);
        v[i] = nan;
        nan_drops += base ? 100 : 0;   // the base case must be a drop for the check to mean anything
        nan_drops += gsr::may_touch_rect(v[0], v[1], v[2], v[3], v[4], v[5], 8.f, 8.f, 15.f, 15.f) ? 0 : 1;
    }
    printf("{\"cases\": %ld, \"misses\": %ld, \"counted\": %ld, \"kept_new\": %ld, \"kept_4edge\": %ld, \"new_not_4edge\": %ld, "
           "\"4edge_not_new\": %ld, \"nan_drops\": %d, \"regions\": [%ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld], \"rho_above_0.99\": %ld, "
           "\"one_pixel\": %ld, \"one_row\": %ld, \"one_column\": %ld, \"opacity_near_1_255\": %ld, \"razor_edge\": %ld}\n",
           cases, misses, counted, kept_new, kept_old, new_not_old, old_not_new, nan_drops, region_n[0], region_n[1], region_n[2], region_n[3],
           region_n[4], region_n[5], region_n[6], region_n[7], region_n[8], rho_999, one_px, one_row, one_col, near_255, razor);
    return misses == 0 && nan_drops == 0 ? 0 : 1;
}
