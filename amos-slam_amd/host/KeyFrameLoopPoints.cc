// KeyFrameLoopPoints.cc -- host side of ORB_SLAM2::SearchByProjection(pKF, Scw, ...): the call of the C ABI on the calling thread's matcher
// handle; nothing of the search is computed here.
#include "KeyFrameLoopPoints.h"

namespace ORB_SLAM2
{

int SearchLoopPointsView(const amos_frame_view &kf, const amos_map_point *points, int nPoints, const amos_loop_points_query &query,
                         const int32_t *matched, const uint8_t *found, const float *scaleFactors, int nLevels, int32_t *loopMatch,
                         amos_loop_points_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    return amos_match_loop_points(h, &kf, points, nPoints, &query, matched, found, nullptr, 0, scaleFactors, nLevels, loopMatch, stats) == AMOS_OK ? 0 : -1;
}

}  // namespace ORB_SLAM2
