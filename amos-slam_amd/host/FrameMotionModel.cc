// FrameMotionModel.cc -- host side of ORB_SLAM2::SearchByMotionModel: the call of the C ABI on the calling thread's matcher handle; nothing is
// computed here.
#include "FrameMotionModel.h"

#include "FrameLocalPoints.h"  // ThreadMatcherHandle

namespace ORB_SLAM2
{

int SearchByMotionModelArrays(const amos_keypoint *keysUn, const uint8_t *descriptors, const float *uRight, int N, const amos_last_point *points,
                              int nPoints, const amos_motion_camera &camera, const float *scaleFactors, int nLevels, float minX, float maxX,
                              float minY, float maxY, amos_proj_query *query, uint8_t *projected, int32_t *match, amos_motion_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    if (amos_match_motion_model(h, keysUn, descriptors, uRight, N, points, nPoints, &camera, scaleFactors, nLevels, minX, maxX, minY, maxY, query,
                                projected, match, stats) != AMOS_OK)
        return -1;
    return stats->n_matches;
}

}  // namespace ORB_SLAM2
