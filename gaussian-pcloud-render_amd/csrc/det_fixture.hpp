// det_fixture.hpp -- the input of the ordered reductions' self-tests (det_backward.hip) and the host sum they are compared with.
// Plain host C++ (tests/det_fixture_main.cpp checks it without a device): sorted keys with runs, positions ascending and distinct
// inside each run as the stable sort leaves them, random flag words and values.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace gsr {

struct DetFixture {
    static constexpr int P = 997, N = 20011;
    // the run lengths at which the walk changes its course: a batch of sixteen elements cut short (cnt < 16), exactly full, or
    // followed by another; slots read in one group of eight (k0 = 0) or two.  These runs come first, so one starts at element 0.
    static constexpr int FORCED[11] = {1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48};
    std::vector<uint32_t> key, val, flags;   // [N] Gaussian ids, ascending; [N] positions, a permutation of [0, N); [N] flag words by position
    std::vector<float> values;               // [N][4][WORDS] slots for WORDS = 16, 8 or 4: the same floats read at the width asked for
    uint32_t unmarked_id = 0;                // the run none of whose quadrants is marked (the forced run of 17): its sums are zeros
    uint32_t x = 2463534242u;
    uint32_t rnd() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; }
    float value() { return (float)((int)(rnd() % 2000001u) - 1000000) * 1.37e-4f * (float)(1u + rnd() % 1000u); }

    DetFixture() : key(N), val(N), flags(N), values((size_t)N * 4 * 16)
    {
        // the forced runs, then runs of 1..80 elements until all N are taken (the last run ends with element N - 1); gaps between
        // the ids, and ids behind the last run, are Gaussians without a run
        int used = 0, runs = 0;
        for (uint32_t id = rnd() % 3u; used < N; id += 1u + (rnd() % 4u == 0u), runs++) {
            const int len = runs < 11 ? FORCED[runs] : 1 + (int)(rnd() % 80u);
            if (len == 17 && runs < 11) unmarked_id = id;
            for (int j = 0; j < len && used < N; j++) key[used++] = id;
        }
        // positions: a strided walk through [0, N) keeps them distinct
        for (int j = 0; j < N; j++) val[j] = (uint32_t)(((uint64_t)j * 7919u) % (uint32_t)N);
        for (int a = 0, b = 0; a < N; a = b) {
            for (b = a; b < N && key[b] == key[a];) b++;
            std::sort(val.begin() + a, val.begin() + b);
        }
        for (int j = 0; j < N; j++) {
            const uint32_t r = rnd();
            flags[j] = ((r & 1u) ? 0x01u : 0u) | ((r & 2u) ? 0x0100u : 0u) | ((r & 4u) ? 0x010000u : 0u) | ((r & 8u) ? 0x01000000u : 0u);
        }
        for (int j = 0; j < N; j++)
            if (key[j] == unmarked_id) flags[val[j]] = 0u;
        for (auto& v : values) v = value();
    }

    // [P][words]: per run and word, the marked quadrants 0..3 of the run's positions in order, added in float64 and rounded once --
    // the additions of k_det_reduce (words = 16) and k_det_reduce_x<words>, one by one; -1 for a Gaussian without a run
    std::vector<float> sums(int words) const
    {
        std::vector<float> out((size_t)P * words, -1.f);
        for (int a = 0, b = 0; a < N; a = b) {
            for (b = a; b < N && key[b] == key[a];) b++;
            for (int c = 0; c < words; c++) {
                double acc = 0.0;
                for (int j = a; j < b; j++)
                    for (int q = 0; q < 4; q++)
                        if ((flags[val[j]] >> (8 * q)) & 0xFFu) acc = acc + (double)values[((size_t)val[j] * 4 + q) * words + c];
                out[(size_t)key[a] * words + c] = (float)acc;
            }
        }
        return out;
    }
};

}  // namespace gsr
