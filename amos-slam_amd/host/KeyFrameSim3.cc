// KeyFrameSim3.cc -- host side of ORB_SLAM2::DeviceSim3Solver: the call of the C ABI on the calling thread's matcher handle; nothing is
// computed here.
#include "KeyFrameSim3.h"

#include "FrameLocalPoints.h"  // ThreadMatcherHandle

namespace ORB_SLAM2
{

int Sim3Arrays(const amos_keypoint *keys1, const amos_sim3_point *points1, int n1, const amos_keypoint *keys2, const amos_sim3_point *points2, int n2,
               const amos_sim3_camera *cameras, const int32_t *match12, const float *levelSigma2, int nLevels, const amos_sim3_params &params,
               void *state, amos_sim3_result *result, uint8_t *inlier, int32_t *matchOut)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    return amos_match_sim3(h, keys1, points1, n1, keys2, points2, n2, cameras, match12, levelSigma2, nLevels, &params, state, result, inlier,
                           matchOut) == AMOS_OK ? 0 : -1;
}

size_t Sim3StateBytes(int n1) { return amos_sim3_state_bytes(n1 > 1 ? n1 : 1); }

}  // namespace ORB_SLAM2
