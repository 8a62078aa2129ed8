// adam_step.hip -- the optimizer step of a training iteration (include/gsr.h gsr_adam_step, gsr_visible_from_radii).
//
// An elementwise, bandwidth-bound pass: 28 B per updated element (read p, g, m, v; write p, m, v), nothing shared between elements, so
// there is no LDS, no atomic and no cross-lane traffic, and every element's result depends on its own four inputs, its row's mask byte
// and the call's constants alone -- which lane, workgroup, path (dwordx4 or scalar) or call computes it does not enter.
//
//   k_adam_step            ONE launch for the 1..8 parameter groups of a cloud.  The group table (adam_step.hpp) travels by value in the
//                          kernel arguments; a workgroup finds its group from the table's prefix of block counts, a choice that is
//                          uniform over the workgroup (scalar selects, no divergence).  Inside its group a workgroup walks rounds of
//                          ADAM_BLOCK_ELEMS elements with a grid stride: 16 B per lane and array on the flat [P * width] arrays.  A
//                          4-vector may span rows (widths 1, 3, 45), so the mask is applied per component; a vector none of whose rows is
//                          visible loads and stores nothing (but its zeros, with zero_grads).  Groups whose four arrays are not all
//                          16-B aligned take the scalar path, as do the last n % 4 elements of an aligned group.
//   k_visible_from_radii   visible[i] = any_v(radii[v][i] > 0): one lane per Gaussian, V coalesced reads, one byte written.
//
// Built with -ffp-contract=off: one rounding per written operation; division and square root are the correctly rounded ones.
#include "adam_step.hpp"
#include "host.hpp"

namespace gsr {

struct AdamConst {
    float b1, b2, c1, c2, eps, rsq2, step;
};

// the definition, per element (include/gsr.h states it formula by formula)
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamConst& c)
{
    m = c.b1 * m + c.c1 * g;
    v = c.b2 * v + c.c2 * (g * g);
    p = p - c.step * (m / (sqrtf(v) * c.rsq2 + c.eps));
}

template <bool MASK>
__device__ __forceinline__ void adam_scalar(const AdamGroupDev& g, const AdamConst& c, const uint8_t* visible, int zero_grads, size_t e)
{
    if (!MASK || visible[(uint32_t)e / g.width] != 0) {
        float p = g.param[e], m = g.exp_avg[e], v = g.exp_avg_sq[e];
        adam_element(p, g.grad[e], m, v, c);
        g.param[e] = p;
        g.exp_avg[e] = m;
        g.exp_avg_sq[e] = v;
    }
    if (zero_grads) g.grad[e] = 0.f;
}

template <bool MASK>
__global__ __launch_bounds__(ADAM_THREADS) void k_adam_step(AdamTable t, const uint8_t* __restrict__ visible)
{
    // this workgroup's group: static indices into the by-value table, selected by a workgroup-uniform comparison
    AdamGroupDev g = t.g[0];
    uint32_t first = 0;
#pragma unroll
    for (int k = 1; k < ADAM_MAX_GROUPS; k++) {
        if (k < t.G && blockIdx.x >= t.g[k - 1].block_end) {
            g = t.g[k];
            first = t.g[k - 1].block_end;
        }
    }
    const AdamConst c{t.b1, t.b2, t.c1, t.c2, t.eps, t.rsq2, g.step};
    const size_t block = blockIdx.x - first, nblocks = g.block_end - first;
    const size_t n = g.n;

    if (!g.vec) {
        for (size_t base = block * ADAM_BLOCK_ELEMS; base < n; base += nblocks * ADAM_BLOCK_ELEMS) {
#pragma unroll
            for (int k = 0; k < ADAM_VEC; k++) {
                const size_t e = base + (size_t)k * ADAM_THREADS + threadIdx.x;
                if (e < n) adam_scalar<MASK>(g, c, visible, t.zero_grads, e);
            }
        }
        return;
    }

    const size_t nvec = n / ADAM_VEC;
    const size_t slots = nvec + (n % ADAM_VEC ? 1 : 0);   // the last slot is the scalar tail
    float4* const P4 = reinterpret_cast<float4*>(g.param);
    float4* const G4 = reinterpret_cast<float4*>(g.grad);
    float4* const M4 = reinterpret_cast<float4*>(g.exp_avg);
    float4* const V4 = reinterpret_cast<float4*>(g.exp_avg_sq);
    for (size_t i = block * ADAM_THREADS + threadIdx.x; i < slots; i += nblocks * ADAM_THREADS) {
        if (i == nvec) {
            for (size_t e = nvec * ADAM_VEC; e < n; e++) adam_scalar<MASK>(g, c, visible, t.zero_grads, e);
            continue;
        }
        uint32_t vis = 0xFu;   // bit k: component k's row is visible
        if (MASK) {
            const uint32_t e0 = (uint32_t)i * ADAM_VEC;
            uint32_t row = e0 / g.width, rem = e0 - row * g.width;
            if (rem + ADAM_VEC <= g.width) {
                vis = visible[row] != 0 ? 0xFu : 0u;
            } else {
                vis = 0;
#pragma unroll
                for (int k = 0; k < ADAM_VEC; k++) {
                    vis |= (visible[row] != 0 ? 1u : 0u) << k;
                    if (++rem == g.width) {
                        rem = 0;
                        if (k < ADAM_VEC - 1) row++;
                    }
                }
            }
        }
        if (vis) {
            const float4 p0 = P4[i], g0 = G4[i], m0 = M4[i], v0 = V4[i];
            float4 p = p0, m = m0, v = v0;
            adam_element(p.x, g0.x, m.x, v.x, c);
            adam_element(p.y, g0.y, m.y, v.y, c);
            adam_element(p.z, g0.z, m.z, v.z, c);
            adam_element(p.w, g0.w, m.w, v.w, c);
            if (MASK && vis != 0xFu) {   // rows that stay keep their bits
                if (!(vis & 1u)) { p.x = p0.x; m.x = m0.x; v.x = v0.x; }
                if (!(vis & 2u)) { p.y = p0.y; m.y = m0.y; v.y = v0.y; }
                if (!(vis & 4u)) { p.z = p0.z; m.z = m0.z; v.z = v0.z; }
                if (!(vis & 8u)) { p.w = p0.w; m.w = m0.w; v.w = v0.w; }
            }
            P4[i] = p;
            M4[i] = m;
            V4[i] = v;
        }
        if (t.zero_grads) G4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__global__ __launch_bounds__(ADAM_THREADS) void k_visible_from_radii(int V, int P, const int* __restrict__ radii,
                                                                     uint8_t* __restrict__ visible)
{
    for (size_t i = (size_t)blockIdx.x * ADAM_THREADS + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * ADAM_THREADS) {
        int any = 0;
        for (int v = 0; v < V; v++) any |= radii[(size_t)v * (size_t)P + i] > 0 ? 1 : 0;
        visible[i] = (uint8_t)any;
    }
}

int launch_visible_from_radii(const Launch& L, int V, int P, const int* radii, uint8_t* visible)
{
    const int64_t blocks = div_up(P, ADAM_THREADS);
    const dim3 grid((unsigned)(blocks < ADAM_MAX_BLOCKS ? blocks : ADAM_MAX_BLOCKS));
    hipLaunchKernelGGL(k_visible_from_radii, grid, dim3(ADAM_THREADS), 0, L.stream, V, P, radii, visible);
    return check_launch(L, "visible_from_radii");
}

int launch_adam_step(const Launch& L, const AdamTable& t, const uint8_t* visible)
{
    const dim3 grid(t.g[t.G - 1].block_end);
    if (visible) hipLaunchKernelGGL(k_adam_step<true>, grid, dim3(ADAM_THREADS), 0, L.stream, t, visible);
    else hipLaunchKernelGGL(k_adam_step<false>, grid, dim3(ADAM_THREADS), 0, L.stream, t, visible);
    return check_launch(L, "adam_step");
}

}  // namespace gsr
