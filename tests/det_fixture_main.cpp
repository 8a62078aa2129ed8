// Host check of the fixture of the ordered reductions' self-tests (csrc/det_fixture.hpp), the very header det_backward.hip includes:
//     g++ -O2 -std=c++17 -I gaussian-pcloud-render_amd/csrc tests/det_fixture_main.cpp -o det_fixture && ./det_fixture
// (an ordinary host program: also fit for -fsanitize=address,undefined).  It checks that the fixture holds the cases the self-tests
// rely on and that DetFixture::sums agrees, bit for bit, with a sum written another way (one pass over the elements, sixteen
// running sums); it prints one line of JSON and returns 0 when everything holds.
#include <stdio.h>
#include <string.h>

#include "det_fixture.hpp"

using gsr::DetFixture;

int main()
{
    const DetFixture F;
    const int N = DetFixture::N, P = DetFixture::P;
    int bad = 0;
    const auto expect = [&](bool ok, const char* what) {
        if (!ok) {
            fprintf(stderr, "det_fixture: %s\n", what);
            bad++;
        }
    };
    expect((int)F.key.size() == N && (int)F.val.size() == N && (int)F.flags.size() == N && F.values.size() == (size_t)N * 64, "array sizes");
    // runs: ids ascending and < P; positions ascending inside a run and a permutation of [0, N) over all
    std::vector<int> run_len, seen(N, 0);
    std::vector<uint32_t> run_id;
    bool sorted = true, ascending = true;
    for (int j = 0; j < N; j++) {
        if (j == 0 || F.key[j] != F.key[j - 1]) {
            sorted = sorted && (j == 0 || F.key[j] > F.key[j - 1]);
            run_len.push_back(0);
            run_id.push_back(F.key[j]);
        } else {
            ascending = ascending && F.val[j] > F.val[j - 1];
        }
        run_len.back()++;
        if (F.val[j] < (uint32_t)N) seen[F.val[j]]++;
    }
    expect(sorted && F.key[N - 1] < (uint32_t)P, "ids ascending and below P");
    expect(ascending, "positions ascending inside every run");
    expect(std::count(seen.begin(), seen.end(), 1) == N, "positions are a permutation of [0, N)");
    // the forced runs come first (so one of them starts at element 0); the last run ends with element N - 1 by construction
    bool forced = run_len.size() > 11;
    for (int r = 0; forced && r < 11; r++) forced = run_len[r] == DetFixture::FORCED[r];
    expect(forced, "the forced run lengths 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48");
    int longest = 0, without_run = P - (int)run_len.size(), gaps = 0;
    for (size_t r = 0; r < run_len.size(); r++) {
        longest = std::max(longest, run_len[r]);
        if (r > 0 && run_id[r] > run_id[r - 1] + 1) gaps++;
    }
    expect(longest > 64 && longest <= 80, "random runs up to 80 elements");
    expect(gaps > 0 && run_id.back() + 1 < (uint32_t)P, "Gaussians without a run between the runs and behind the last");
    // the run without a mark: seventeen elements, every flag word zero; every other run has marks
    int unmarked_runs = 0;
    for (int a = 0, b = 0; a < N; a = b) {
        uint32_t any = 0;
        for (b = a; b < N && F.key[b] == F.key[a]; b++) any |= F.flags[F.val[b]];
        if (any == 0) {
            unmarked_runs++;
            expect(F.key[a] == F.unmarked_id && b - a == 17, "the unmarked run is the forced run of 17");
        }
    }
    expect(unmarked_runs == 1, "exactly one run without a mark");
    // the reference sum at the three slot widths against one pass over the elements
    for (int words : {16, 8, 4}) {
        const std::vector<float> got = F.sums(words);
        std::vector<float> want((size_t)P * words, -1.f);
        double acc[16] = {};
        for (int j = 0; j < N; j++) {
            if (j == 0 || F.key[j] != F.key[j - 1])
                for (double& a : acc) a = 0.0;
            const uint32_t pos = F.val[j];
            for (int q = 0; q < 4; q++)
                if (F.flags[pos] & (0xFFu << (8 * q)))
                    for (int c = 0; c < words; c++) acc[c] += (double)F.values[((size_t)pos * 4 + q) * words + c];
            for (int c = 0; c < words; c++) want[(size_t)F.key[j] * words + c] = (float)acc[c];
        }
        expect(got.size() == want.size() && memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0, "sums() against the one-pass sum");
        const float zero = 0.f;
        bool zeros = true;
        for (int c = 0; c < words; c++) zeros = zeros && memcmp(&got[(size_t)F.unmarked_id * words + c], &zero, 4) == 0;
        expect(zeros, "the unmarked run's sums are +0, not the -1 of an untouched row");
        size_t untouched = 0;
        for (int g = 0; g < P; g++) untouched += got[(size_t)g * words] == -1.f && !std::binary_search(run_id.begin(), run_id.end(), (uint32_t)g);
        expect((int)untouched == without_run, "rows of Gaussians without a run stay -1");
    }
    printf("{\"runs\": %zu, \"longest\": %d, \"without_run\": %d, \"failed\": %d}\n", run_len.size(), longest, without_run, bad);
    return bad != 0;
}
