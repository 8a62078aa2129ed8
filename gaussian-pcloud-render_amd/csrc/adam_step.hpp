// adam_step.hpp -- the work split and the by-value group table of the fused Adam step (adam_step.hip), shared by
// the kernels, the entries of api.hip and -- the constants -- the tests, which read them from this file.
#pragma once
#include "common.hpp"

namespace gsr {

constexpr int ADAM_VEC = 4;            // floats per lane and access: 16 B, global_load_dwordx4 / global_store_dwordx4
constexpr int ADAM_THREADS = 256;      // lanes per workgroup, both kernels
constexpr int ADAM_BLOCK_ELEMS = ADAM_VEC * ADAM_THREADS;   // elements of one group a workgroup covers per grid-stride round
constexpr int ADAM_MAX_GROUPS = 8;
constexpr int ADAM_MAX_BLOCKS = 8192;  // grid cap over all groups of a call: 256 CUs x 8 workgroups x 4 rounds in flight

// One parameter group as the kernel sees it.  n = P * width < 2^31 elements; byte offsets reach 2^33 and are 64-bit in the kernel.
struct AdamGroupDev {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint32_t n;           // elements
    uint32_t width;       // elements per row (per Gaussian)
    uint32_t block_end;   // prefix of block counts: this group's workgroups are blockIdx.x in [previous block_end, block_end)
    uint32_t vec;         // 1: all four arrays 16-B aligned, dwordx4 path (scalar tail for n % 4); 0: the scalar path throughout
    float step;           // lr / (1 - beta1^t), formed in double, rounded once
};

// The kernel's whole argument besides the mask: travels by value in the kernel arguments (8 x 56 B + 32 B)
struct AdamTable {
    AdamGroupDev g[ADAM_MAX_GROUPS];
    int G;
    float b1, b2, c1, c2;   // beta1, beta2, 1.0f - beta1, 1.0f - beta2
    float eps, rsq2;        // eps; 1 / sqrt(1 - beta2^t), formed in double, rounded once
    int zero_grads;
};

// workgroups of a group of n elements when the call's groups hold `units` rounds of ADAM_BLOCK_ELEMS in total: every round its own
// workgroup below the cap, a proportional share (at least one) above it
inline uint32_t adam_group_blocks(int64_t n, int64_t units)
{
    const int64_t mine = div_up(n, ADAM_BLOCK_ELEMS);
    if (units <= ADAM_MAX_BLOCKS) return (uint32_t)mine;
    const int64_t share = mine * ADAM_MAX_BLOCKS / units;
    return (uint32_t)(share < 1 ? 1 : share);
}

int launch_visible_from_radii(const Launch& L, int V, int P, const int* radii, uint8_t* visible);
int launch_adam_step(const Launch& L, const AdamTable& t, const uint8_t* visible);

}  // namespace gsr
