// FramePoseOptimization.cc -- host side of ORB_SLAM2::PoseOptimization: the call of the C ABI on the calling thread's matcher handle; nothing
// is computed here.
#include "FramePoseOptimization.h"

#include "FrameLocalPoints.h"  // ThreadMatcherHandle

namespace ORB_SLAM2
{

int PoseOptimizationArrays(const amos_keypoint *keysUn, const float *uRight, int N, int32_t *match, const float *pointsXyz, const uint8_t *hasObs,
                           int nPoints, const amos_pose_camera &camera, const float *invLevelSigma2, int nLevels, bool clearOutliers,
                           uint8_t *outlier, amos_pose_result *result)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    if (amos_match_pose_optimization(h, keysUn, uRight, N, match, pointsXyz, hasObs, nPoints, &camera, invLevelSigma2, nLevels, clearOutliers ? 1 : 0,
                                     outlier, result) != AMOS_OK)
        return -1;
    return result->n_inliers;
}

}  // namespace ORB_SLAM2
