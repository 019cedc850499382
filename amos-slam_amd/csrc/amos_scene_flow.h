// amos_scene_flow.h -- the back-projection of Tracking::GetSceneFlowObj (src/Tracking.cc:955-990): a LAST-frame pixel with its depth to
// the world through mLastFrame.mTcw (pre_3d), the depth lookup of a tracked point, the current pixel to the world (cur_3d), the flow
// norm, and the distance from an epipolar line (:928-946, 1141-1152).  The one copy of this arithmetic: k_epipolar and k_scene_flow_3d
// (amos_flow.hip), k_fmat_keep (amos_fmat.hip), k_pnp_points (amos_pnp.hip) and k_dyna_tail (amos_dyna.hip) call it.
#pragma once
#include "amos_common.h"

namespace amos {

struct SceneFlowArgs {
    float cx, cy, invfx, invfy;
    float Rwl[9], twl[3];  // last camera -> world (Rlw^T, -Rlw^T tlw as floats, Tracking.cc:970-973)
    float Rwc[9], Ow[3];   // current camera -> world (Frame::mRwc, mOw)
};

inline SceneFlowArgs scene_flow_args(const amos_scene_flow_camera *cam)
{
    SceneFlowArgs a;
    a.cx = cam->cx; a.cy = cam->cy; a.invfx = cam->invfx; a.invfy = cam->invfy;
    // Rwl = Rlw^T, twl = -Rlw^T * tlw (one gemm, alpha = -1: double accumulation, one rounding)
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) a.Rwl[3 * r + c] = cam->Tlw[4 * c + r];
        a.twl[r] = (float)(-((double)cam->Tlw[r] * cam->Tlw[3] + (double)cam->Tlw[4 + r] * cam->Tlw[7] + (double)cam->Tlw[8 + r] * cam->Tlw[11]));
    }
    for (int k = 0; k < 9; k++) a.Rwc[k] = cam->Rwc[k];
    for (int k = 0; k < 3; k++) a.Ow[k] = cam->Ow[k];
    return a;
}

__device__ __forceinline__ float gemm_row(const float *R, int r, float x, float y, float z, float t)
{
    return (float)((double)R[3 * r] * x + (double)R[3 * r + 1] * y + (double)R[3 * r + 2] * z + (double)t);
}

// :960-961 and x3Dp = Rwl * x3Dp + twl: pre_3d of the last-frame pixel (x, y) with depth z1
__device__ __forceinline__ void scene_flow_pre3d(const SceneFlowArgs &a, float x, float y, float z1, float &p0, float &p1, float &p2)
{
    const float xl = __fmul_rn(__fmul_rn(__fsub_rn(x, a.cx), z1), a.invfx);
    const float yl = __fmul_rn(__fmul_rn(__fsub_rn(y, a.cy), z1), a.invfy);
    p0 = gemm_row(a.Rwl, 0, xl, yl, z1, a.twl[0]);
    p1 = gemm_row(a.Rwl, 1, xl, yl, z1, a.twl[1]);
    p2 = gemm_row(a.Rwl, 2, xl, yl, z1, a.twl[2]);
}

// the two depths of a tracked point (P in the last frame, Q in the current one) at its truncated coordinates; a pixel outside the
// width x height maps has no depth (0).  k_pnp_points calls it; k_dyna_tail keeps the same lines written out (the reason is there).
__device__ __forceinline__ void scene_flow_depths(const float *depthLast, size_t lastStride, const float *depthCur, size_t curStride, int width, int height,
                                                  float2 P, float2 Q, float &z1, float &z2)
{
    const int x1 = (int)P.x, y1 = (int)P.y, x2 = (int)Q.x, y2 = (int)Q.y;
    const bool in1 = P.x >= 0 && P.y >= 0 && x1 < width && y1 < height, in2 = Q.x >= 0 && Q.y >= 0 && x2 < width && y2 < height;
    z1 = in1 ? depthLast[(size_t)y1 * lastStride + x1] : 0.f;
    z2 = in2 ? depthCur[(size_t)y2 * curStride + x2] : 0.f;
}

// :1160-1164: cur_3d of the current-frame pixel (x, y) through (Rwc, Ow); the reference scales the CURRENT pixel by z1 and stacks z2:
// restated as written
__device__ __forceinline__ void scene_flow_cur3d(const SceneFlowArgs &a, const float *Rwc, const float *Ow, float x, float y, float z1, float z2, float &c0,
                                                 float &c1, float &c2)
{
    const float xc = __fmul_rn(__fmul_rn(__fsub_rn(x, a.cx), z1), a.invfx);
    const float yc = __fmul_rn(__fmul_rn(__fsub_rn(y, a.cy), z1), a.invfy);
    c0 = gemm_row(Rwc, 0, xc, yc, z2, Ow[0]);
    c1 = gemm_row(Rwc, 1, xc, yc, z2, Ow[1]);
    c2 = gemm_row(Rwc, 2, xc, yc, z2, Ow[2]);
}

// sf_norm uses x and z only (:1176).  std::sqrt(float) is correctly rounded; the device's single-precision square root is not, the
// double one is, and rounding a double square root of a float to float is exact (53 >= 2 * 24 + 2 bits)
__device__ __forceinline__ float scene_flow_norm(float p0, float p2, float c0, float c2)
{
    const float fx = __fsub_rn(p0, c0), fz = __fsub_rn(p2, c2);
    return (float)__dsqrt_rn((double)__fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fz, fz)));
}

// dd of Tracking.cc:930-935: the distance of q from the epipolar line F p, |q . (F p)| / sqrt(A^2 + B^2) in doubles;
// A = F00 * x + F01 * y + F02 evaluated left to right, no fused multiply-add
__device__ __forceinline__ double epipolar_distance(const double *F, float px_, float py_, float qx_, float qy_)
{
    const double px = px_, py = py_, qx = qx_, qy = qy_;
    const double A = __dadd_rn(__dadd_rn(__dmul_rn(F[0], px), __dmul_rn(F[1], py)), F[2]);
    const double B = __dadd_rn(__dadd_rn(__dmul_rn(F[3], px), __dmul_rn(F[4], py)), F[5]);
    const double C = __dadd_rn(__dadd_rn(__dmul_rn(F[6], px), __dmul_rn(F[7], py)), F[8]);
    const double num = fabs(__dadd_rn(__dadd_rn(__dmul_rn(A, qx), __dmul_rn(B, qy)), C));
    return __ddiv_rn(num, __dsqrt_rn(__dadd_rn(__dmul_rn(A, A), __dmul_rn(B, B))));
}

}  // namespace amos
