// render_math_main.cpp -- stand-alone host check of the forward kernels' two arithmetic modes (csrc/render_math.hpp).
// Built and run by tests/test_cpu_render_math_host.py:
//     g++ -O2 -std=c++17 -ffp-contract=off -I gaussian-pcloud-render_amd/csrc tests/render_math_main.cpp -o render_math
//     ./render_math [draws = 4194304] [seed = 1]
// (an ordinary host program: also fit for -fsanitize=address,undefined).  It prints one line of JSON.
//
// The header is the very text the kernels compile; here its value type is float and the host's exp2f STANDS IN for the device's
// v_exp_f32 (1 ulp), in the exact form (inside exp_nonpos) and in the fast one alike.  What the hardware's exp2 does is covered by the
// GPU tests, not here.
//
// Seeded random (conic, offset, opacity) draws:
//   conics     inverted in float32 from sigma_1, sigma_2 log-uniform in [0.3, 30] pixels and a correlation rho uniform in [-0.95, 0.95];
//   pixels     integer coordinates in [0, 4000]^2;
//   centres    the pixel plus an offset of Mahalanobis length r uniform in [0, 4] in a uniform direction (one draw in 64 sits exactly on
//              the pixel), rounded to float32; the kernels' d = centre - pixel is formed in float32 from that;
//   opacities  uniform in (0, 1], a quarter of them placed so that alpha falls within a few percent of the 1/255 cut.
// A draw is KEPT when its float64 alpha = o exp(power), from the float32 inputs, lies in [1/255, 0.99) (the clamp itself is the same
// operation in both modes).  For the kept draws:
//   max / mean relative error of the exact form's alpha and of the fast form's against float64;
//   disagreements between !(p2 > 0) and !(power > 0) (the skip each mode takes);
//   zero-opacity twins (the padding of an odd pair, opacity 0) whose alpha is not exactly 0, in either mode.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "render_math.hpp"

struct Rng {
    uint64_t s;
    uint64_t next()
    {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)
    double uni(double lo, double hi) { return lo + (hi - lo) * uni(); }
};

int main(int argc, char** argv)
{
    const long draws = argc > 1 ? atol(argv[1]) : (1l << 22);
    Rng rng{argc > 2 ? (uint64_t)atoll(argv[2]) : 1ull};
    const double PI = 3.14159265358979323846;
    long kept = 0, sign_disagree = 0, twin_nonzero = 0, near_cut = 0, on_pixel = 0, far_pixel = 0, small_sigma = 0, big_sigma = 0, high_rho = 0;
    double max_exact = 0, max_fast = 0, sum_exact = 0, sum_fast = 0;
    for (long i = 0; i < draws; i++) {
        const double s1 = 0.3 * std::pow(100.0, rng.uni()), s2 = 0.3 * std::pow(100.0, rng.uni()), rho = rng.uni(-0.95, 0.95);
        // the covariance and its inverse in float32, the way the preprocess kernel forms a conic (a c - b^2, then three divisions)
        const float a = (float)(s1 * s1), b = (float)(rho * s1 * s2), c = (float)(s2 * s2);
        const float det = a * c - b * b;
        if (!(det > 0.f)) continue;
        const float A = c / det, B = -b / det, C = a / det;
        const int px = (int)(rng.next() % 4001u), py = (int)(rng.next() % 4001u);
        const bool centred = (rng.next() & 63u) == 0;
        const double r = centred ? 0.0 : rng.uni(0.0, 4.0), th = rng.uni(0.0, 2 * PI);
        // offset = L (r cos th, r sin th) with L L^T the covariance: Mahalanobis length r
        const double u = r * std::cos(th), v = r * std::sin(th);
        const double ox = s1 * u, oy = s2 * (rho * u + std::sqrt(1 - rho * rho) * v);
        const float mx = (float)((double)px + ox), my = (float)((double)py + oy);
        const float dx = mx - (float)px, dy = my - (float)py;
        const double dxd = (double)mx - px, dyd = (double)my - py;
        const double power64 = -0.5 * ((double)A * dxd * dxd + (double)C * dyd * dyd) - (double)B * dxd * dyd;
        float o;
        const bool razor = (rng.next() & 3u) == 0;
        if (razor) o = (float)(rng.uni(0.97, 1.08) / 255.0 / std::exp(power64));
        else o = (float)(1.0 - rng.uni());
        if (!(o > 0.f && o <= 1.f)) continue;
        const double alpha64 = (double)o * std::exp(power64);
        if (!(alpha64 >= 1.0 / 255.0 && alpha64 < 0.99)) continue;
        kept++;
        near_cut += alpha64 < 1.05 / 255.0;
        on_pixel += dx == 0.f && dy == 0.f;
        far_pixel += px > 3000 || py > 3000;
        small_sigma += s1 < 1.0 || s2 < 1.0;
        big_sigma += s1 > 10.0 || s2 > 10.0;
        high_rho += std::fabs(rho) > 0.9;

        // exact mode: the unfolded conic
        const float power = gsr::power_exact(A, B, C, dx, dy);
        const float a_exact = gsr::alpha_exact(o, power);
        // fast mode: the conic folded once (at staging), then p2 and the bare exp2
        const float Ap = gsr::fold_square_term(A), Bp = gsr::fold_cross_term(B), Cp = gsr::fold_square_term(C);
        const float p2 = gsr::power2_fast(Ap, Bp, Cp, dx, dy);
        const float a_fast = gsr::alpha_fast(o, p2);

        const double e_exact = std::fabs((double)a_exact - alpha64) / alpha64, e_fast = std::fabs((double)a_fast - alpha64) / alpha64;
        if (e_exact > max_exact) max_exact = e_exact;
        if (e_fast > max_fast) max_fast = e_fast;
        sum_exact += e_exact;
        sum_fast += e_fast;
        sign_disagree += (!(power > 0.0f)) != (!(p2 > 0.0f));
        // the second half of a lone survivor's pair: the same record at opacity 0 must give alpha = 0 exactly (the 1/255 test drops it)
        const float t_exact = gsr::alpha_exact(0.f, power), t_fast = gsr::alpha_fast(0.f, p2);
        twin_nonzero += !(t_exact == 0.f) || !(t_fast == 0.f) || !(t_fast < 1.0f / 255.0f);
    }
    printf("{\"draws\": %ld, \"kept\": %ld, \"max_rel_exact\": %.6e, \"max_rel_fast\": %.6e, \"mean_rel_exact\": %.6e, \"mean_rel_fast\": %.6e, "
           "\"sign_disagree\": %ld, \"twin_nonzero\": %ld, \"near_cut\": %ld, \"on_pixel\": %ld, \"far_pixel\": %ld, \"small_sigma\": %ld, "
           "\"big_sigma\": %ld, \"high_rho\": %ld}\n",
           draws, kept, max_exact, max_fast, kept ? sum_exact / kept : 0.0, kept ? sum_fast / kept : 0.0, sign_disagree, twin_nonzero, near_cut,
           on_pixel, far_pixel, small_sigma, big_sigma, high_rho);
    return 0;
}
