// density_control.hpp -- the work split, the scratch plan and the by-value tables of adaptive density control (density_control.hip,
// DESIGN.md section 4j), shared by the kernels, the entries of api.hip and -- the constants -- the tests, which read them from this file.
#pragma once
#include "common.hpp"

namespace gsr {

constexpr int DENSITY_THREADS = 256;      // lanes per workgroup, every kernel; the plan's kernels take one Gaussian per lane
constexpr int DENSITY_SCAN_ROUND = 256;   // workgroup counts the one scanning workgroup takes per round of its loop
constexpr int DENSITY_VEC = 4;            // floats per lane and access of the 16-B path
constexpr int DENSITY_BLOCK_ELEMS = DENSITY_VEC * DENSITY_THREADS;   // output elements of one group a workgroup covers per round
constexpr int DENSITY_MAX_GROUPS = 8;
constexpr int DENSITY_MAX_BLOCKS = 8192;  // grid cap of the gather over all groups of a call
constexpr int DENSITY_COUNTS = 4;         // arrays of workgroup counts: rows (the scan turns them into bases), carried, copies, gone

inline int64_t density_blocks(int P) { return div_up(P > 0 ? P : 1, DENSITY_THREADS); }
// the scratch of gsr_density_plan: DENSITY_COUNTS arrays of one uint32 per workgroup of the decide kernel
inline size_t density_scratch_bytes(int P) { return align_up((size_t)DENSITY_COUNTS * (size_t)density_blocks(P) * sizeof(uint32_t), 256); }

// The rule as the kernels see it: gsr_density_rule, by value in the kernel arguments.
struct DensityRuleDev {
    float grad_threshold, dense_size, min_opacity, max_world_size;
    int max_screen_radius, log_scales, normalize_rotations;
    uint32_t key0, key1;   // the low and the high half of seed
};

// One group of a gather as the kernel sees it.  n = P_out * width < 2^31 output elements.
struct DensityGroupDev {
    const float* src;
    float* dst;
    uint32_t n;           // output elements
    uint32_t width;       // elements per row
    uint32_t block_end;   // prefix of block counts: this group's workgroups are blockIdx.x in [previous block_end, block_end)
    uint32_t vec;         // 1: src and dst 16-B aligned, width a multiple of 4 and the role COPY or MOMENT: the 16-B path
    int role;             // GSR_DENSITY_COPY / MEANS / SCALES / MOMENT
};
struct DensityTable {
    DensityGroupDev g[DENSITY_MAX_GROUPS];
    int G;
};

// workgroups of a group of n output elements when the call's groups hold `units` rounds of DENSITY_BLOCK_ELEMS in total
inline uint32_t density_group_blocks(int64_t n, int64_t units)
{
    const int64_t mine = div_up(n, DENSITY_BLOCK_ELEMS);
    if (units <= DENSITY_MAX_BLOCKS) return (uint32_t)mine;
    const int64_t share = mine * DENSITY_MAX_BLOCKS / units;
    return (uint32_t)(share < 1 ? 1 : share);
}

struct DensityPlanArgs {
    int P;
    const float* scales;
    const float* opacities;
    const float* grad_norm_sum;
    const int* visible_views;
    const int* max_radius;
    const uint8_t* prune_mask;   // or NULL
    uint32_t* offsets;           // [P + 1]
    uint8_t* action;             // [P]
    int64_t* totals;             // [5]
    uint32_t* counts;            // the scratch: [DENSITY_COUNTS][density_blocks(P)]
};
struct DensityApplyArgs {
    int P;
    uint32_t P_out;
    const uint32_t* offsets;
    const uint8_t* action;
    const float* scales;      // [P][3], MEANS groups
    const float* rotations;   // [P][4], MEANS groups
    const float* noise;       // [P][2][3] or NULL: the generator
    int32_t* index;           // [P_out] or NULL
};

int launch_density_plan(const Launch& L, const DensityRuleDev& r, const DensityPlanArgs& a);
int launch_density_apply(const Launch& L, const DensityRuleDev& r, const DensityTable& t, const DensityApplyArgs& a);

}  // namespace gsr
