// cloud_geometry.hpp -- the work split and the scratch plan of the point-cloud neighbourhood kernels (cloud_geometry.hip, DESIGN.md
// section 4k), shared by the kernels, their entries and -- the constants -- the tests, which read them from this file.
#pragma once
#include "common.hpp"

namespace gsr {

constexpr int CLOUD_THREADS = 256;        // lanes per workgroup of the per-point kernels
constexpr int CLOUD_RUN = 64;             // sorted points per fine box: one wave answers the queries of one run
constexpr int CLOUD_COARSE = 64;          // fine boxes per coarse box (4 096 points)
constexpr int CLOUD_BOX_WORDS = 8;        // a box: lo xyz, hi xyz, two spare words (the cloud's box: present count, spare)
constexpr int CLOUD_MAX_PARTS = 1024;     // grid cap of the first reduction stage
constexpr int CLOUD_MAX_K = 32;
constexpr int CLOUD_KEY_BITS = 31;        // 30 Morton bits, bit 30 set for an absent point
constexpr uint32_t CLOUD_ABSENT_KEY = 1u << 30;
constexpr int CLOUD_JACOBI_SWEEPS = GSR_CLOUD_JACOBI_SWEEPS;

inline bool cloud_sizes_ok(int P, int K) { return P >= 1 && P < (1 << 30) && K >= 1 && K <= CLOUD_MAX_K; }
inline int64_t cloud_runs(int P) { return div_up(P, CLOUD_RUN); }
inline int64_t cloud_coarse(int P) { return div_up(cloud_runs(P), CLOUD_COARSE); }
inline int cloud_parts(int P) { const int64_t b = div_up(P, CLOUD_THREADS); return (int)(b < CLOUD_MAX_PARTS ? b : CLOUD_MAX_PARTS); }

// The scratch of gsr_knn, carved in this order, every array on a 256-B boundary.
struct KnnScratch {
    float* parts;        // [cloud_parts][CLOUD_BOX_WORDS] per-workgroup boxes and present counts
    float* box;          // [CLOUD_BOX_WORDS] the cloud's box; word 6 holds the number of present points (uint32 bits)
    uint32_t* key[2];    // [P] Morton keys, ping-pong
    uint32_t* val[2];    // [P] point indices, ping-pong
    uint32_t* hist;      // the sort's count matrix
    uint32_t* totals;    // [RADIX]
    float4* sorted;      // [P] (x, y, z, index bits) in Morton order
    float* fine;         // [cloud_runs][CLOUD_BOX_WORDS]
    float* coarse;       // [cloud_coarse][CLOUD_BOX_WORDS]
    size_t bytes;
};
inline KnnScratch knn_scratch(void* base, int P)
{
    KnnScratch s;
    char* cur = reinterpret_cast<char*>(base);
    const auto carve = [&cur](auto*& p, size_t count) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(cur);
        cur += align_up(count * sizeof(*p), 256);
    };
    const size_t n = (size_t)P;
    carve(s.parts, (size_t)cloud_parts(P) * CLOUD_BOX_WORDS);
    carve(s.box, (size_t)CLOUD_BOX_WORDS);
    carve(s.key[0], n);
    carve(s.key[1], n);
    carve(s.val[0], n);
    carve(s.val[1], n);
    carve(s.hist, (size_t)RADIX * (size_t)sort_hist_stride(P));
    carve(s.totals, (size_t)RADIX);
    carve(s.sorted, n);
    carve(s.fine, (size_t)cloud_runs(P) * CLOUD_BOX_WORDS);
    carve(s.coarse, (size_t)cloud_coarse(P) * CLOUD_BOX_WORDS);
    s.bytes = (size_t)(cur - reinterpret_cast<char*>(base));
    return s;
}
// (K does not enter: the lists live in registers.  It stays an argument of the size query so that a layout that needs it can come.)
inline size_t knn_scratch_bytes(int P, int K) { (void)K; return knn_scratch(nullptr, P).bytes; }

struct CloudGeometryArgs {
    int P, K, k_s, k_n;
    const float* points;
    const int32_t* knn_idx;
    int oriented;
    float ox, oy, oz;
    float* spacing;
    float* cov6;
    float* eigenvalues;
    float* normals;
    float* rotations;
};

int launch_knn(const Launch& L, int P, const float* points, int K, int32_t* idx, float* d2, const KnnScratch& s);
int launch_cloud_geometry(const Launch& L, const CloudGeometryArgs& a);

}  // namespace gsr
