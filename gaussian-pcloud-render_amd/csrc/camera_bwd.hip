// camera_bwd.hip -- dL/d{viewmatrix, projmatrix, campos} of every view, from the gradient records a backward left in the arenas.
//
// k_preprocess_backward pushes a view's render-level sums (dL/d mean2D, conic, colour: the 64-B records) through the projection
// chain to the Gaussian and adds over the views.  The camera gradient is the same chain taken to the other operand and added over
// the Gaussians of ONE view.  Notation of preprocess_bwd.hip's header; m = (x, y, z, 1) the mean, r_k = (view[k], view[4+k],
// view[8+k]) the rows of the view rotation, t_k = r_k . mean + view[12+k]:
//
//   conic      da, db, dc, dm0, dm1 and dt = (dtx, dty, dtz) by k_preprocess_backward's expressions -- dtx = 0 (dty = 0) where the
//              frustum clamp was active, tx and ty taken as constants in dtz: the reference's convention (its Dn != 0 guard
//              answers a float32 overflow of det^2 that float64 does not have).
//              m0 = J00 r0 + J02 r2, m1 = J11 r1 + J12 r2, so
//                  dL/dr0 += J00 dm0 + dtx mean      dL/dr1 += J11 dm1 + dty mean      dL/dr2 += J02 dm0 + J12 dm1 + dtz mean
//                  dL/dview[12+k] += dt_k
//   mean2D     ndc = (h0, h1) / (h3 + 1e-7), h_k = sum_j proj[k + 4j] m_j.  With iw = 1 / (h3 + 1e-7) and (gx, gy) the record's words:
//                  gh0 = gx iw,  gh1 = gy iw,  gh3 = -(h0 iw^2 gx + h1 iw^2 gy),      dL/dproj[k + 4j] += gh_k m_j   (k = 0, 1, 3)
//   SH colour  depends on mean - campos only: dL/dcampos -= (what sh_backward adds to the mean)
//
// view[3, 7, 11, 15] and proj[2, 6, 10, 14] are never read by the forward: their gradients are written as +0.
//
// The conic chain (3D covariance -> a, b, c -> da, db, dc -> dL/dr_k, dL/dt) is evaluated in float64 from the float32 inputs and
// records: for a splat next to the camera its terms cancel several hundredfold, and in float32 one such splat put a whole view's
// dL/dviewmatrix several 1e-4 of its largest entry off (the randomised sweep, tests/test_gpu_camera_fuzz.py, cases 0, 40, 47).  The
// frustum-clamp decisions stay the forward's float32 ones.  The mean2D and SH terms are evaluated in float32 (one rounding per
// written operation, like the rest of the library).  Every term is ADDED in float64, in an
// order that depends on nothing but the sizes: a thread's Gaussians by ascending index, a butterfly over the wave's 64 lanes, the
// four waves through LDS, the workgroups' partials by ascending block index in a second launch.  No atomics, no hand-off between
// workgroups: the result does not depend on when which workgroup runs.
#include "common.hpp"
#include "splat_math.hpp"
#include "sh_bwd.hpp"

namespace gsr {

struct CamArgs {
    int P, M, nblk, V;
    float tanfovx, tanfovy, focal_x, focal_y, scale_modifier;
    const float *means3D, *shs, *scales, *rotations, *cov3D_precomp;
    const float *view, *proj, *campos;   // [V][16], [V][16], [V][3]
    const int* radii;                    // [V][P]
    const uint8_t* clamped;
    const float* grad_rec;
    size_t g_stride, gr_stride;
    double* slab;                        // [V][nblk][CAM_SLAB_WORDS]
};

// Sum of acc[i] over the workgroup's CAM_THREADS threads, in a fixed order: xor butterfly over the 64 lanes (every lane ends with
// the same sum: IEEE addition commutes), then (wave 0 + wave 1) + (wave 2 + wave 3).  Returns term `threadIdx.x` to the first
// CAM_TERMS threads and 0 to the others.  s_part: [CAM_THREADS / 64][CAM_SLAB_WORDS] doubles.
__device__ __forceinline__ double cam_block_sum(double (&acc)[CAM_TERMS], double* s_part)
{
    static_assert(CAM_THREADS == 256, "the cross-wave tree below is written for four waves");
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < CAM_TERMS; i++) {
        double x = acc[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
        if (lane == 0) s_part[wave * CAM_SLAB_WORDS + i] = x;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t >= (uint32_t)CAM_TERMS) return 0.0;
    return (s_part[t] + s_part[CAM_SLAB_WORDS + t]) + (s_part[2 * CAM_SLAB_WORDS + t] + s_part[3 * CAM_SLAB_WORDS + t]);
}

// acc: 0..2 dL/dr0, 3..5 dL/dr1, 6..8 dL/dr2, 9..11 dL/dt; 12..15 gh0 m, 16..19 gh1 m, 20..23 gh3 m; 24..26 dL/dcampos.
// DEG: the active SH degree, 0 also without SHs (a degree-0 colour does not depend on the view direction)
template <int DEG>
__global__ __launch_bounds__(CAM_THREADS) void k_camera_partials(CamArgs a)
{
    __shared__ double s_part[(CAM_THREADS / 64) * CAM_SLAB_WORDS];
    // Workgroup order (speed only, any order gives the same bits): the V views of one block of Gaussians are taken by V consecutive
    // workgroups of one residue class mod 8 -- what this part hands to one XCD -- so that views 1 .. V - 1 find the block's cloud
    // inputs in that XCD's L2.
    const uint32_t seq = blockIdx.x >> 3, vw = seq % a.V, blk = (seq / a.V) * 8 + (blockIdx.x & 7u);
    if (blk >= (uint32_t)a.nblk) return;            // (the whole workgroup: nblk is rounded up to a multiple of 8 in the grid)
    double acc[CAM_TERMS];
#pragma unroll
    for (int i = 0; i < CAM_TERMS; i++) acc[i] = 0.0;

    const float* view = a.view + 16 * vw;
    const float* proj = a.proj + 16 * vw;
    const float fx = a.focal_x, fy = a.focal_y;
    const float* rec_v = at_view(a.grad_rec, a.gr_stride, vw);
    const int* radii_v = a.radii + (size_t)vw * a.P;

#pragma unroll 1
    for (int k = 0; k < CAM_G; k++) {
        const int64_t row = (int64_t)blk * CAM_ROWS + k * CAM_THREADS + threadIdx.x;
        if (row >= a.P) break;                      // rows ascend with k: nothing further for this thread
        const int idx = (int)row;
        if (!(radii_v[idx] > 0)) continue;          // invisible in this view: exact zeros

        const float* recp = rec_v + (size_t)idx * GRAD_REC_WORDS;
        const float4 rec0 = *reinterpret_cast<const float4*>(recp);
        const float4 rec1 = *reinterpret_cast<const float4*>(recp + 4);
        const V3 mean = v3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
        // ---- conic -> (a, b, c) -> rows of M -> view rows, in DOUBLE from the float32 inputs.  A splat next to the camera and beyond
        // the frustum clamp has a c / det of 40 .. 170 and a conic gradient that cancels several hundredfold in da / db / dc: in
        // float32 its term alone was off by up to 1e-3 of itself, a few 1e-4 of the whole view's gradient (tests/test_gpu_camera_fuzz.py).
        // Only the clamp decisions are the forward's float32 ones (cov2d_project): that is the function the forward evaluated.
        double S[6];
        if (a.cov3D_precomp) {
#pragma unroll
            for (int i = 0; i < 6; i++) S[i] = (double)a.cov3D_precomp[6 * (size_t)idx + i];
        } else {
            const float4 q4 = *reinterpret_cast<const float4*>(a.rotations + 4 * (size_t)idx);
            const double r = q4.x, x = q4.y, y = q4.z, z = q4.w, md = (double)a.scale_modifier;
            const double s0 = md * (double)a.scales[3 * idx], s1 = md * (double)a.scales[3 * idx + 1], s2 = md * (double)a.scales[3 * idx + 2];
            const double v0 = s0 * s0, v1 = s1 * s1, v2 = s2 * s2;
            // R from the raw quaternion (quat_to_cols), Sigma = R diag(s^2) R^T
            const double R00 = 1.0 - 2.0 * (y * y + z * z), R01 = 2.0 * (x * y - r * z), R02 = 2.0 * (x * z + r * y);
            const double R10 = 2.0 * (x * y + r * z), R11 = 1.0 - 2.0 * (x * x + z * z), R12 = 2.0 * (y * z - r * x);
            const double R20 = 2.0 * (x * z - r * y), R21 = 2.0 * (y * z + r * x), R22 = 1.0 - 2.0 * (x * x + y * y);
            S[0] = R00 * R00 * v0 + R01 * R01 * v1 + R02 * R02 * v2;
            S[1] = R00 * R10 * v0 + R01 * R11 * v1 + R02 * R12 * v2;
            S[2] = R00 * R20 * v0 + R01 * R21 * v1 + R02 * R22 * v2;
            S[3] = R10 * R10 * v0 + R11 * R11 * v1 + R12 * R12 * v2;
            S[4] = R10 * R20 * v0 + R11 * R21 * v1 + R12 * R22 * v2;
            S[5] = R20 * R20 * v0 + R21 * R21 * v1 + R22 * R22 * v2;
        }
        const float limx = 1.3f * a.tanfovx, limy = 1.3f * a.tanfovy;
        const V3 tf = xform_point_4x3(mean, view);     // the forward's float32 view-space mean: its clamp decisions
        const float txtz_f = tf.x / tf.z, tytz_f = tf.y / tf.z;
        const bool clamp_x = txtz_f < -limx || txtz_f > limx, clamp_y = tytz_f < -limy || tytz_f > limy;
        const double mx = mean.x, my = mean.y, mz = mean.z, fxd = fx, fyd = fy;
        const double r0[3] = {view[0], view[4], view[8]}, r1[3] = {view[1], view[5], view[9]}, r2[3] = {view[2], view[6], view[10]};
        const double tz = r2[0] * mx + r2[1] * my + r2[2] * mz + (double)view[14];
        const double iz = 1.0 / tz, iz2 = iz * iz, iz3 = iz2 * iz;      // (one float64 division here, one for Dn: they are the slow part)
        const double txz = (r0[0] * mx + r0[1] * my + r0[2] * mz + (double)view[12]) * iz;
        const double tyz = (r1[0] * mx + r1[1] * my + r1[2] * mz + (double)view[13]) * iz;
        const double tx = fmin((double)limx, fmax(-(double)limx, txz)) * tz, ty = fmin((double)limy, fmax(-(double)limy, tyz)) * tz;
        const double J00 = fxd * iz, J02 = -(fxd * tx) * iz2, J11 = fyd * iz, J12 = -(fyd * ty) * iz2;
        double m0[3], m1[3], u[3], w[3], dm0[3], dm1[3];
#pragma unroll
        for (int j = 0; j < 3; j++) { m0[j] = J00 * r0[j] + J02 * r2[j]; m1[j] = J11 * r1[j] + J12 * r2[j]; }
        u[0] = S[0] * m0[0] + S[1] * m0[1] + S[2] * m0[2]; u[1] = S[1] * m0[0] + S[3] * m0[1] + S[4] * m0[2];
        u[2] = S[2] * m0[0] + S[4] * m0[1] + S[5] * m0[2];
        w[0] = S[0] * m1[0] + S[1] * m1[1] + S[2] * m1[2]; w[1] = S[1] * m1[0] + S[3] * m1[1] + S[4] * m1[2];
        w[2] = S[2] * m1[0] + S[4] * m1[1] + S[5] * m1[2];
        const double ca = (m0[0] * u[0] + m0[1] * u[1] + m0[2] * u[2]) + (double)0.3f;
        const double cb = m0[0] * w[0] + m0[1] * w[1] + m0[2] * w[2];
        const double cc = (m1[0] * w[0] + m1[1] * w[1] + m1[2] * w[2]) + (double)0.3f;
        const double gA = rec0.z, gB = rec0.w, gC = rec1.x;
        const double det = ca * cc - cb * cb;
        const double Dn = 1.0 / ((det * det) + (double)0.0000001f);
        const double da = Dn * (-cc * cc * gA + 2 * cb * cc * gB + (det - ca * cc) * gC);
        const double dc = Dn * (-ca * ca * gC + 2 * ca * cb * gB + (det - ca * cc) * gA);
        const double db = Dn * 2 * (cb * cc * gA - (det + 2 * cb * cb) * gB + ca * cb * gC);
#pragma unroll
        for (int j = 0; j < 3; j++) { dm0[j] = (2 * da) * u[j] + db * w[j]; dm1[j] = (2 * dc) * w[j] + db * u[j]; }
        const double dJ00 = r0[0] * dm0[0] + r0[1] * dm0[1] + r0[2] * dm0[2], dJ02 = r2[0] * dm0[0] + r2[1] * dm0[1] + r2[2] * dm0[2];
        const double dJ11 = r1[0] * dm1[0] + r1[1] * dm1[1] + r1[2] * dm1[2], dJ12 = r2[0] * dm1[0] + r2[1] * dm1[1] + r2[2] * dm1[2];
        const double dtx = clamp_x ? 0.0 : -fxd * iz2 * dJ02;
        const double dty = clamp_y ? 0.0 : -fyd * iz2 * dJ12;
        const double dtz = -(fxd * dJ00 + fyd * dJ11) * iz2 + 2 * (fxd * tx * dJ02 + fyd * ty * dJ12) * iz3;
        const double md3[3] = {mx, my, mz};
#pragma unroll
        for (int j = 0; j < 3; j++) {
            acc[j] += J00 * dm0[j] + dtx * md3[j];
            acc[3 + j] += J11 * dm1[j] + dty * md3[j];
            acc[6 + j] += (J02 * dm0[j] + J12 * dm1[j]) + dtz * md3[j];
        }
        acc[9] += dtx; acc[10] += dty; acc[11] += dtz;

        // ---- mean2D -> the three rows of proj the perspective divide reads
        {
            const float hx = proj[0] * mean.x + proj[4] * mean.y + proj[8] * mean.z + proj[12];
            const float hy = proj[1] * mean.x + proj[5] * mean.y + proj[9] * mean.z + proj[13];
            const float hw = ((proj[3] * mean.x + proj[7] * mean.y) + proj[11] * mean.z) + proj[15];
            const float iw = 1.0f / (hw + 0.0000001f);
            const float kx = hx * iw * iw, ky = hy * iw * iw;
            const float gx = rec0.x, gy = rec0.y;
            const float gh0 = gx * iw, gh1 = gy * iw, gh3 = -(kx * gx + ky * gy);
            acc[12] += (double)(gh0 * mean.x); acc[13] += (double)(gh0 * mean.y); acc[14] += (double)(gh0 * mean.z); acc[15] += (double)gh0;
            acc[16] += (double)(gh1 * mean.x); acc[17] += (double)(gh1 * mean.y); acc[18] += (double)(gh1 * mean.z); acc[19] += (double)gh1;
            acc[20] += (double)(gh3 * mean.x); acc[21] += (double)(gh3 * mean.y); acc[22] += (double)(gh3 * mean.z); acc[23] += (double)gh3;
        }

        // ---- colour -> view direction -> campos
        if constexpr (DEG > 0) {
            constexpr int NSH = sh_words<DEG>();
            float shv[NSH], unused[NSH];
            const float* shp = a.shs + (size_t)idx * a.M * 3;
#pragma unroll
            for (int i = 0; i < NSH; i++) { shv[i] = shp[i]; unused[i] = 0.f; }
            const V3 cam = v3(a.campos[3 * vw], a.campos[3 * vw + 1], a.campos[3 * vw + 2]);
            const uint8_t cm = at_view(a.clamped, a.g_stride, vw)[idx];
            const V3 ddir = sh_backward<DEG>(mean, cam, shv, cm, v3(rec1.y, rec1.z, rec1.w), unused);
            acc[24] -= (double)ddir.x; acc[25] -= (double)ddir.y; acc[26] -= (double)ddir.z;
        }
    }

    const double tot = cam_block_sum(acc, s_part);
    if (threadIdx.x < (uint32_t)CAM_SLAB_WORDS)    // 27 sums and 5 zeros: the whole 256-B line
        a.slab[((size_t)vw * a.nblk + blk) * CAM_SLAB_WORDS + threadIdx.x] = tot;
}

// One workgroup per view: thread t adds the partials of blocks t, t + CAM_THREADS, ... in ascending order, cam_block_sum adds the
// threads, one rounding to float32, and all 35 entries of the view are written.
__global__ __launch_bounds__(CAM_THREADS) void k_camera_sum(int nblk, int with_campos, const double* __restrict__ slab,
                                                            float* __restrict__ dL_dview, float* __restrict__ dL_dproj,
                                                            float* __restrict__ dL_dcampos)
{
    __shared__ double s_part[(CAM_THREADS / 64) * CAM_SLAB_WORDS];
    __shared__ float s_out[CAM_SLAB_WORDS];
    const uint32_t vw = blockIdx.x, t = threadIdx.x;
    double acc[CAM_TERMS];
#pragma unroll
    for (int i = 0; i < CAM_TERMS; i++) acc[i] = 0.0;
    for (int b = (int)t; b < nblk; b += CAM_THREADS) {
        const double* row = slab + ((size_t)vw * nblk + b) * CAM_SLAB_WORDS;
#pragma unroll
        for (int i = 0; i < CAM_TERMS; i++) acc[i] += row[i];
    }
    const double tot = cam_block_sum(acc, s_part);
    if (t < (uint32_t)CAM_TERMS) s_out[t] = (float)tot;
    __syncthreads();
    if (t < 16) {            // view[k + 4 j]: row k of the rotation (j < 3) or of the translation (j = 3); row 3 is never read
        const uint32_t k = t & 3u, j = t >> 2;
        dL_dview[16 * vw + t] = k == 3 ? 0.f : j < 3 ? s_out[3 * k + j] : s_out[9 + k];
    } else if (t < 32) {     // proj[k + 4 j]: rows 0, 1, 3 (preprocess never reads row 2)
        const uint32_t e = t - 16, k = e & 3u, j = e >> 2;
        dL_dproj[16 * vw + e] = k == 2 ? 0.f : s_out[12 + 4 * (k == 3 ? 2 : k) + j];
    } else if (t < 35) {
        dL_dcampos[3 * vw + (t - 32)] = with_campos ? s_out[24 + (t - 32)] : 0.f;
    }
}

int launch_camera_partials(const Launch& L, const gsr_params& p, const Batch& B, const int* radii, double* slab)
{
    CamArgs a;
    a.P = p.P; a.M = p.M; a.nblk = camera_blocks(p.P); a.V = B.V;
    a.tanfovx = p.tanfovx; a.tanfovy = p.tanfovy;
    a.focal_y = p.H / (2.0f * p.tanfovy);
    a.focal_x = p.W / (2.0f * p.tanfovx);
    a.scale_modifier = p.scale_modifier;
    a.means3D = p.means3D; a.shs = p.shs; a.scales = p.scales; a.rotations = p.rotations;
    a.cov3D_precomp = p.cov3D_precomp; a.view = p.viewmatrix; a.proj = p.projmatrix; a.campos = p.campos;
    a.radii = radii; a.clamped = B.g.clamped;
    a.grad_rec = B.grad_rec; a.g_stride = B.g_stride; a.gr_stride = B.gr_stride;
    a.slab = slab;
    const dim3 grid((unsigned)(div_up(a.nblk, 8) * 8 * B.V)), block(CAM_THREADS);
    switch (p.shs ? p.D : 0) {
    case 0: hipLaunchKernelGGL(k_camera_partials<0>, grid, block, 0, L.stream, a); break;
    case 1: hipLaunchKernelGGL(k_camera_partials<1>, grid, block, 0, L.stream, a); break;
    case 2: hipLaunchKernelGGL(k_camera_partials<2>, grid, block, 0, L.stream, a); break;
    default: hipLaunchKernelGGL(k_camera_partials<3>, grid, block, 0, L.stream, a); break;
    }
    return check_launch(L, "camera_partials");
}

int launch_camera_sum(const Launch& L, int V, int P, int with_campos, const double* slab, float* dL_dview, float* dL_dproj,
                      float* dL_dcampos)
{
    hipLaunchKernelGGL(k_camera_sum, dim3((unsigned)V), dim3(CAM_THREADS), 0, L.stream, camera_blocks(P), with_campos, slab, dL_dview,
                       dL_dproj, dL_dcampos);
    return check_launch(L, "camera_sum");
}

}  // namespace gsr
