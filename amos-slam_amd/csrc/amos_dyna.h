// amos_dyna.h -- the per-point arithmetic of the tail of Tracking::GetSceneFlowObj (src/Tracking.cc:1012-1184): the reprojection
// error of a match under a 3 x 4 float pose, Frame::SetPose's camera centre, and the scene flow under the chosen pose (the depth lookup and
// the epipolar distance are amos_scene_flow.h).  For k_dyna_tail (amos_dyna.hip); restated once more in tests/dyna_restatement.py.  Plain + - * / sqrt in the written order (the library
// builds with -ffp-contract=off).
#pragma once
#include "amos_common.h"
#include "amos_pnp_core.h"
#include "amos_scene_flow.h"

namespace amos {
namespace dyna {

// :1031-1063 for one point.  cv::projectPoints(x3D, Rodrigues(R), t, K, 0) is evaluated with R itself (no Rodrigues round trip,
// DESIGN.md section 2): the pose's floats as doubles, pnp::point_error's projection (z ? 1 / z : 1, u and v stored as float), then
// Rpe = std::sqrt(du * du + dv * dv) in float.  P = rows of [R | t].  The float square root is taken as the correctly rounded double
// square root of the float, rounded to float (exact, as in k_scene_flow_3d).
__device__ __forceinline__ float rpe(const float *P, float X, float Y, float Z, float u, float v, double fx, double fy, double cx, double cy)
{
    const double M[12] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10], P[3], P[7], P[11]};
    return (float)__dsqrt_rn((double)pnp::point_error(M, X, Y, Z, u, v, fx, fy, cx, cy));
}

// Frame::SetPose -> UpdatePoseMatrices: Rwc = Rcw^T, Ow = -Rcw^T * tcw (one gemm, alpha = -1: double accumulation, one rounding -- the
// twl of scene_flow_args)
__device__ __forceinline__ void set_pose(const float *P, float *Rwc, float *Ow)
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rwc[3 * r + c] = P[4 * c + r];
        Ow[r] = (float)(-((double)P[r] * P[3] + (double)P[4 + r] * P[7] + (double)P[8 + r] * P[11]));
    }
}

// :1153-1183: sf_norm of a match whose two depths are positive, cur_3d through (Rwc, Ow) of the chosen pose; the current pixel is
// scaled by z1, as the reference writes it (the pieces k_scene_flow_3d is made of, amos_scene_flow.h)
__device__ __forceinline__ float sf_norm(const SceneFlowArgs &a, const float *Rwc, const float *Ow, float px, float py, float qx, float qy,
                                         float z1, float z2)
{
    float p0, p1, p2, c0, c1, c2;
    scene_flow_pre3d(a, px, py, z1, p0, p1, p2);
    scene_flow_cur3d(a, Rwc, Ow, qx, qy, z1, z2, c0, c1, c2);
    return scene_flow_norm(p0, p2, c0, c2);
}

}  // namespace dyna
}  // namespace amos
