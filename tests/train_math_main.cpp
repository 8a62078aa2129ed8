// train_math_main.cpp -- stand-alone host check of what the fast render BACKWARD adds to csrc/render_math.hpp (gsr_set_train_math).
// Built and run by tests/test_cpu_train_math_host.py:
//     g++ -O2 -std=c++17 -ffp-contract=off -I gaussian-pcloud-render_amd/csrc tests/train_math_main.cpp -o train_math
//     ./train_math [draws = 4194304] [seed = 1]
// (an ordinary host program: also fit for -fsanitize=address,undefined).  It prints one line of JSON.
//
// The header is the very text the kernels compile; the host's exp2f stands in for v_exp_f32, in the forward's form and in the
// backward's alike.  The draws are those of tests/render_math_main.cpp: sigma 0.3 - 30 px log-uniform, |rho| <= 0.95, pixel coordinates
// to 4000, offsets of Mahalanobis length up to 4, a quarter of the opacities placed within a few percent of the 1/255 cut.  Here EVERY
// draw with a valid conic and opacity counts (not only those whose alpha lies in [1/255, 0.99)): the backward has to take the forward's
// decision on both sides of each cut.
//   (a) alpha_fast_g(o, p2, G) -- the backward's form, which hands out G = 2^p2 for the G dL/dalpha weight -- against alpha_fast(o, p2),
//       the forward's: alpha bit for bit, G = rm_exp2(p2) bit for bit, and the same hit decision !(p2 > 0) && !(alpha < 1/255);
//   (b) the flush's unfolding of the staged conic: unfold(fold(x)) within 3e-7 relative of x for the three conic terms (four roundings
//       of 2^-24: two products and two rounded constants), and the doubling inside it exact.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv)
{
    const long draws = argc > 1 ? atol(argv[1]) : (1l << 22);
    Rng rng{argc > 2 ? (uint64_t)atoll(argv[2]) : 1ull};
    const double PI = 3.14159265358979323846;
    long used = 0, alpha_differs = 0, g_differs = 0, hit_differs = 0, hits = 0, misses_alpha = 0, misses_sign = 0, clamped = 0, near_cut = 0;
    long twice_inexact = 0;
    double max_unfold = 0;
    for (long i = 0; i < draws; i++) {
        const double s1 = 0.3 * std::pow(100.0, rng.uni()), s2 = 0.3 * std::pow(100.0, rng.uni()), rho = rng.uni(-0.95, 0.95);
        const float a = (float)(s1 * s1), b = (float)(rho * s1 * s2), c = (float)(s2 * s2);
        const float det = a * c - b * b;
        if (!(det > 0.f)) continue;
        const float A = c / det, B = -b / det, C = a / det;
        const int px = (int)(rng.next() % 4001u), py = (int)(rng.next() % 4001u);
        const bool centred = (rng.next() & 63u) == 0;
        const double r = centred ? 0.0 : rng.uni(0.0, 4.0), th = rng.uni(0.0, 2 * PI);
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
        used++;
        const double alpha64 = (double)o * std::exp(power64);
        near_cut += alpha64 > 0.95 / 255.0 && alpha64 < 1.05 / 255.0;

        // the staging lane's fold (forward and backward alike), then the forward's form and the backward's
        const float Ap = gsr::fold_square_term(A), Bp = gsr::fold_cross_term(B), Cp = gsr::fold_square_term(C);
        const float p2 = gsr::power2_fast(Ap, Bp, Cp, dx, dy);
        const float a_fwd = gsr::alpha_fast(o, p2);
        float G = -1.f;
        const float a_bwd = gsr::alpha_fast_g(o, p2, G);
        alpha_differs += bits(a_fwd) != bits(a_bwd);
        g_differs += bits(G) != bits(gsr::rm_exp2(p2));
        const bool hit_fwd = !(p2 > 0.0f) && !(a_fwd < 1.0f / 255.0f), hit_bwd = !(p2 > 0.0f) && !(a_bwd < 1.0f / 255.0f);
        hit_differs += hit_fwd != hit_bwd;
        hits += hit_fwd;
        misses_alpha += !(p2 > 0.0f) && a_fwd < 1.0f / 255.0f;
        misses_sign += p2 > 0.0f;
        clamped += a_fwd == 0.99f;

        // (b) the flush's unfolding
        const float terms[3] = {A, B, C}, folded[3] = {Ap, Bp, Cp};
        for (int k = 0; k < 3; k++) {
            const float back = k == 1 ? gsr::unfold_cross_term(folded[k]) : gsr::unfold_square_term(folded[k]);
            if (terms[k] != 0.f) {
                const double e = std::fabs((double)back - (double)terms[k]) / std::fabs((double)terms[k]);
                if (e > max_unfold) max_unfold = e;
            } else if (back != 0.f) {
                max_unfold = 1.0;
            }
            twice_inexact += (double)gsr::unfold_twice(folded[k]) != 2.0 * (double)folded[k];
        }
    }
    printf("{\"draws\": %ld, \"used\": %ld, \"alpha_differs\": %ld, \"g_differs\": %ld, \"hit_differs\": %ld, \"hits\": %ld, "
           "\"misses_alpha\": %ld, \"misses_sign\": %ld, \"clamped\": %ld, \"near_cut\": %ld, \"max_unfold_rel\": %.6e, \"twice_inexact\": %ld}\n",
           draws, used, alpha_differs, g_differs, hit_differs, hits, misses_alpha, misses_sign, clamped, near_cut, max_unfold, twice_inexact);
    return 0;
}
