// amos_scene_flow.h -- the back-projection of Tracking::GetSceneFlowObj (src/Tracking.cc:955-990): a LAST-frame pixel with its depth to
// the world through mLastFrame.mTcw (pre_3d).  Shared by k_scene_flow_3d (amos_flow.hip) and the PnP's point lists (amos_pnp.hip).
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

}  // namespace amos
