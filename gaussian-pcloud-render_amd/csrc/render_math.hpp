// render_math.hpp -- the per-(pixel, entry) arithmetic of the render kernels, in its two modes (gsr_set_render_math for forwards that
// save nothing; gsr_set_train_math for forwards that save for a backward, and for the render backward that follows them):
//
//   exact (0, the default)   the reference's operations one rounding at a time: power = -0.5 (A dx^2 + C dy^2) - B dx dy,
//                            alpha = min(0.99, o exp(power)) with the bit-exact exp of exp_nonpos, C += (c alpha) T.  Images equal a
//                            strict-order build of the reference bit for bit.
//   fast (1, opt-in)         the same quantities in fewer instructions, every fusion written out (no contraction pragma, the build
//                            stays -ffp-contract=off): the staging lane folds -0.5 log2(e) / -log2(e) into the conic once per entry,
//                            the pixels evaluate p2 = power log2(e) with two multiplies and two fused multiply-adds, alpha =
//                            min(0.99, o 2^p2) with the hardware's v_exp_f32 and no range reduction, and the blend is w = alpha T once
//                            per entry and one fused multiply-add per channel.  As accurate as the exact form against float64
//                            (tests/render_math_main.cpp), rounded elsewhere: within the 1e-4 contract, not bit-identical.
//
// Everything here is __host__ __device__ and written against a value type V -- float, or on the device the register pair f32x2 whose
// operations are the packed fp32 instructions -- so that the host test program compiles the very text the kernels run.  On the host
// exp2f stands in for v_exp_f32.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GSR_HD __host__ __device__ __forceinline__
#else
#define GSR_HD inline
#endif

namespace gsr {

#if defined(__clang__)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
GSR_HD f32x2 rm_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
#endif
GSR_HD float rm_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// 2^x: v_exp_f32 (1 ulp, denormal results flushed) on the device, exp2f on the host
GSR_HD float rm_exp2(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(x);
#else
    return __builtin_exp2f(x);
#endif
}

// ---- exact mode -----------------------------------------------------------------------------------------------------------

template <typename V>
GSR_HD V power_exact(V A, V B, V C, V dx, V dy)
{
    return -0.5f * (A * dx * dx + C * dy * dy) - B * dx * dy;
}

// exp(x) for the compositing loop.  Instruction-for-instruction the core of the ocml expf that `exp(power)` of the
// reference resolves to under hipcc (extended-precision x*log2(e), v_rndne, v_exp_f32, v_ldexp_f32), minus its two
// range clamps: x > 88.7 -> inf and x < -103.3 -> 0.  Neither can change a decision or a blended value: entries
// with power > 0 are skipped before alpha is used, and for x < -103 both forms give a value < 1e-44, far below
// the 1/255 cut for any finite opacity.  For every x in [-103, 0] the result is bit-identical to expf(x).
GSR_HD float exp_nonpos(float x)
{
    const float ph = x * 0x1.715476p+0f;
    float pl = __builtin_fmaf(x, 0x1.715476p+0f, -ph);
    pl = __builtin_fmaf(x, 0x1.4ae0bep-26f, pl);
    const float e = __builtin_rintf(ph);
    const float r = rm_exp2((ph - e) + pl);
    return __builtin_ldexpf(r, (int)e);
}

#if defined(__clang__)
// two-entry version: the multiplies / fused multiply-adds / adds become packed fp32 instructions (v_pk_*_f32, two
// IEEE operations per lane per issue slot); rounding per component is that of exp_nonpos
GSR_HD f32x2 exp_nonpos2(f32x2 x)
{
    const f32x2 c = {0x1.715476p+0f, 0x1.715476p+0f}, cc = {0x1.4ae0bep-26f, 0x1.4ae0bep-26f};
    const f32x2 ph = x * c;
    f32x2 pl = __builtin_elementwise_fma(x, c, -ph);
    pl = __builtin_elementwise_fma(x, cc, pl);
    const f32x2 e = {__builtin_rintf(ph.x), __builtin_rintf(ph.y)};
    const f32x2 a = (ph - e) + pl;
    f32x2 r;
    r.x = __builtin_ldexpf(rm_exp2(a.x), (int)e.x);
    r.y = __builtin_ldexpf(rm_exp2(a.y), (int)e.y);
    return r;
}
#endif

// (one entry; the kernels evaluate two at a time: O2 * exp_nonpos2(power), then the same clamp)
GSR_HD float alpha_exact(float o, float power) { return __builtin_fminf(0.99f, o * exp_nonpos(power)); }

// ---- fast mode ------------------------------------------------------------------------------------------------------------

// once per staged entry: A' = A (-0.5 log2 e), B' = B (-log2 e), C' = C (-0.5 log2 e), float32 products (the footprint test keeps
// reading the unfolded record)
constexpr float RM_NEG_HALF_LOG2E = -0x1.715476p-1f, RM_NEG_LOG2E = -0x1.715476p+0f;
GSR_HD float fold_square_term(float AC) { return AC * RM_NEG_HALF_LOG2E; }   // A and C
GSR_HD float fold_cross_term(float B) { return B * RM_NEG_LOG2E; }

// p2 = power log2(e) = A' dx^2 + B' dx dy + C' dy^2 from the folded conic: two multiplies, two fused multiply-adds.  Its sign is the
// power's up to rounding (both skips stay in their negated form, so a NaN and a 0 * inf behave as in the exact mode).
template <typename V>
GSR_HD V power2_fast(V Ap, V Bp, V Cp, V dx, V dy)
{
    const V s = rm_fma(Cp, dy, Bp * dx);
    return rm_fma(Ap * dx, dx, dy * s);
}

// alpha = min(0.99, o 2^p2): one v_exp_f32, no range reduction, no ldexp (p2 <= 0 for every entry that counts; a result below 2^-126
// is flushed to 0 and is six orders of magnitude under the 1/255 cut either way)
GSR_HD float alpha_fast(float o, float p2) { return __builtin_fminf(0.99f, o * rm_exp2(p2)); }

// The fast render backward (render_bwd.hip RenderBwdFast) needs G = 2^p2 on its own, for the G dL/dalpha weight, beside the alpha:
// the same two operations as alpha_fast with the exponential handed out, so alpha, G and the hit decision are the fast forward's bit
// for bit (tests/train_math_main.cpp pins it to alpha_fast).
GSR_HD float alpha_fast_g(float o, float p2, float& G)
{
    G = rm_exp2(p2);
    return __builtin_fminf(0.99f, o * G);
}
#if defined(__clang__)
// two entries: the product is one packed multiply, rounding per component that of alpha_fast_g
GSR_HD f32x2 alpha_fast_g2(f32x2 o, f32x2 p2, f32x2& G)
{
    G = f32x2{rm_exp2(p2.x), rm_exp2(p2.y)};
    const f32x2 al = o * G;
    return f32x2{__builtin_fminf(0.99f, al.x), __builtin_fminf(0.99f, al.y)};
}
#endif

// The backward's flush shifts the moments to the splat centre with the UNFOLDED conic, and its staged rows hold the folded one (no
// spare row for a second copy): A = (2 A') (-ln 2), B = B' (-ln 2) -- the doubling is exact, and the kernel applies the one rounded
// factor -ln 2 to the per-lane constant that multiplies A Dx + B Dy (resp. B Dx + C Dy) anyway, so unfolding costs an add and a select
// per lane and batch of eight entries.  unfold(fold(x)) is x within four roundings of 2^-24 (two products, two rounded constants); it
// enters gradients held to tolerance only.
constexpr float RM_NEG_LN2 = -0x1.62e43p-1f;
GSR_HD float unfold_twice(float ACp) { return ACp + ACp; }             // A' and C': the part of their unfolding that is exact
GSR_HD float unfold_scale(float v) { return v * RM_NEG_LN2; }         // the common factor
GSR_HD float unfold_square_term(float ACp) { return unfold_scale(unfold_twice(ACp)); }
GSR_HD float unfold_cross_term(float Bp) { return unfold_scale(Bp); }

// C += c w with w = alpha T formed once per entry: one fused multiply-add per channel (packed for a channel pair)
template <typename V>
GSR_HD void blend_fast(V& acc, V c, float w)
{
    acc = rm_fma(c, V(w), acc);
}

}  // namespace gsr
