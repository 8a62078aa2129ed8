// sh_bwd.hpp -- the SH backward of one (view, Gaussian), shared by preprocess_bwd.hip (dL/dSH and the view direction's share of
// dL/dmean) and camera_bwd.hip (the same vector, negated, is the Gaussian's share of dL/dcampos).
#pragma once
#include "splat_math.hpp"

namespace gsr {

// d normalize(v) / dv applied to dv (reference CR/auxiliary.h:107-117)
__device__ __forceinline__ V3 dnormvdv(V3 v, V3 dv)
{
    const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
    const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
    V3 r;
    r.x = ((+sum2 - v.x * v.x) * dv.x - v.y * v.x * dv.y - v.z * v.x * dv.z) * invsum32;
    r.y = (-v.x * v.y * dv.x + (sum2 - v.y * v.y) * dv.y - v.z * v.y * dv.z) * invsum32;
    r.z = (-v.x * v.z * dv.x - v.y * v.z * dv.y + (sum2 - v.z * v.z) * dv.z) * invsum32;
    return r;
}

template <int DEG> constexpr int sh_words() { return 3 * (DEG + 1) * (DEG + 1); }

// SH backward (reference CR/backward.cu:20-139): adds this view's dL_dsh rows into acc, returns the mean gradient through the
// normalised view direction.
template <int deg>
__device__ __forceinline__ V3 sh_backward(V3 pos, V3 campos, const float* sh, uint32_t cmask, V3 dL_dRGB,
                                          float (&acc)[sh_words<deg>()])
{
    const V3 dir_orig = pos - campos;
    const float len = sqrtf(dot3(dir_orig, dir_orig));
    const V3 dir = v3(dir_orig.x / len, dir_orig.y / len, dir_orig.z / len);
    dL_dRGB.x *= (cmask & 1u) ? 0 : 1;
    dL_dRGB.y *= (cmask & 2u) ? 0 : 1;
    dL_dRGB.z *= (cmask & 4u) ? 0 : 1;
    V3 dRGBdx = v3(0, 0, 0), dRGBdy = v3(0, 0, 0), dRGBdz = v3(0, 0, 0);
    const float x = dir.x, y = dir.y, z = dir.z;
#define SHV(k) v3(sh[3 * (k)], sh[3 * (k) + 1], sh[3 * (k) + 2])
#define PUT(k, s) do { const V3 t_ = (s) * dL_dRGB; acc[3 * (k)] += t_.x; acc[3 * (k) + 1] += t_.y; acc[3 * (k) + 2] += t_.z; } while (0)
    PUT(0, kSH_C0);
    if constexpr (deg > 0) {
        PUT(1, -kSH_C1 * y);
        PUT(2, kSH_C1 * z);
        PUT(3, -kSH_C1 * x);
        dRGBdx = -kSH_C1 * SHV(3);
        dRGBdy = -kSH_C1 * SHV(1);
        dRGBdz = kSH_C1 * SHV(2);
        if constexpr (deg > 1) {
            const float xx = x * x, yy = y * y, zz = z * z;
            const float xy = x * y, yz = y * z, xz = x * z;
            PUT(4, kSH_C2[0] * xy);
            PUT(5, kSH_C2[1] * yz);
            PUT(6, kSH_C2[2] * (2.f * zz - xx - yy));
            PUT(7, kSH_C2[3] * xz);
            PUT(8, kSH_C2[4] * (xx - yy));
            dRGBdx = dRGBdx + ((((kSH_C2[0] * y) * SHV(4) + (kSH_C2[2] * 2.f * -x) * SHV(6)) + (kSH_C2[3] * z) * SHV(7)) +
                               (kSH_C2[4] * 2.f * x) * SHV(8));
            dRGBdy = dRGBdy + ((((kSH_C2[0] * x) * SHV(4) + (kSH_C2[1] * z) * SHV(5)) + (kSH_C2[2] * 2.f * -y) * SHV(6)) +
                               (kSH_C2[4] * 2.f * -y) * SHV(8));
            dRGBdz = dRGBdz + (((kSH_C2[1] * y) * SHV(5) + (kSH_C2[2] * 2.f * 2.f * z) * SHV(6)) + (kSH_C2[3] * x) * SHV(7));
            if constexpr (deg > 2) {
                PUT(9, kSH_C3[0] * y * (3.f * xx - yy));
                PUT(10, kSH_C3[1] * xy * z);
                PUT(11, kSH_C3[2] * y * (4.f * zz - xx - yy));
                PUT(12, kSH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy));
                PUT(13, kSH_C3[4] * x * (4.f * zz - xx - yy));
                PUT(14, kSH_C3[5] * z * (xx - yy));
                PUT(15, kSH_C3[6] * x * (xx - 3.f * yy));
                // scalar*vec first, then the remaining scalars left to right (reference CR/backward.cu:99-122)
                V3 s;
                s = (((kSH_C3[0] * SHV(9)) * 3.f) * 2.f) * xy;
                s = s + (kSH_C3[1] * SHV(10)) * yz;
                s = s + ((kSH_C3[2] * SHV(11)) * -2.f) * xy;
                s = s + (((kSH_C3[3] * SHV(12)) * -3.f) * 2.f) * xz;
                s = s + (kSH_C3[4] * SHV(13)) * (-3.f * xx + 4.f * zz - yy);
                s = s + ((kSH_C3[5] * SHV(14)) * 2.f) * xz;
                s = s + ((kSH_C3[6] * SHV(15)) * 3.f) * (xx - yy);
                dRGBdx = dRGBdx + s;
                s = ((kSH_C3[0] * SHV(9)) * 3.f) * (xx - yy);
                s = s + (kSH_C3[1] * SHV(10)) * xz;
                s = s + (kSH_C3[2] * SHV(11)) * (-3.f * yy + 4.f * zz - xx);
                s = s + (((kSH_C3[3] * SHV(12)) * -3.f) * 2.f) * yz;
                s = s + ((kSH_C3[4] * SHV(13)) * -2.f) * xy;
                s = s + ((kSH_C3[5] * SHV(14)) * -2.f) * yz;
                s = s + (((kSH_C3[6] * SHV(15)) * -3.f) * 2.f) * xy;
                dRGBdy = dRGBdy + s;
                s = (kSH_C3[1] * SHV(10)) * xy;
                s = s + (((kSH_C3[2] * SHV(11)) * 4.f) * 2.f) * yz;
                s = s + ((kSH_C3[3] * SHV(12)) * 3.f) * (2.f * zz - xx - yy);
                s = s + (((kSH_C3[4] * SHV(13)) * 4.f) * 2.f) * xz;
                s = s + (kSH_C3[5] * SHV(14)) * (xx - yy);
                dRGBdz = dRGBdz + s;
            }
        }
    }
#undef PUT
#undef SHV
    const V3 dL_ddir = v3(dot3(dRGBdx, dL_dRGB), dot3(dRGBdy, dL_dRGB), dot3(dRGBdz, dL_dRGB));
    return dnormvdv(dir_orig, dL_ddir);
}

}  // namespace gsr
