// KeyFrameSim3Optimize.cc -- host side of ORB_SLAM2::OptimizeSim3: the call of the C ABI on the calling thread's matcher handle; nothing of
// the optimisation is computed here.
#include "KeyFrameSim3Optimize.h"

namespace ORB_SLAM2
{

int OptimizeSim3Arrays(const amos_keypoint *kps1, const amos_sim3_point *points1, int n1, const amos_keypoint *kps2, const amos_sim3_point *points2,
                       int n2, const amos_sim3_camera *cameras, const int32_t *match12, const float *invLevelSigma2, int nLevels,
                       const amos_sim3_opt_pair &pair, int32_t *matchOut, amos_sim3_opt_result *result)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    return amos_match_sim3_optimize(h, kps1, points1, n1, kps2, points2, n2, cameras, match12, invLevelSigma2, nLevels, &pair, matchOut, result) ==
                   AMOS_OK
               ? 0
               : -1;
}

}  // namespace ORB_SLAM2
