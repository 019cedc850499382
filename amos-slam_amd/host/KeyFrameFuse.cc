// KeyFrameFuse.cc -- host side of ORB_SLAM2::Fuse / FuseInNeighbors: the call of the C ABI on the calling thread's matcher handle; nothing of
// the search is computed here.
#include "KeyFrameFuse.h"

namespace ORB_SLAM2
{

int FuseViews(const amos_frame_view *kfs, int nKFs, const amos_map_point *points, int nPoints, int nPairs, const int32_t *pairFrame,
              const int32_t *pointFirst, const int32_t *pointCount, const int32_t *outOff, const amos_fuse_camera *cameras, const uint8_t *skip,
              int nOut, const float *scaleFactors, const float *invLevelSigma2, int nLevels, int mode, amos_window_query *query, uint8_t *inView,
              int32_t *bestIdx, int32_t *bestDist, amos_fuse_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    return amos_match_fuse(h, kfs, nKFs, points, nPoints, nPairs, pairFrame, pointFirst, pointCount, outOff, cameras, skip, nOut, scaleFactors,
                           invLevelSigma2, nLevels, mode, AMOS_TH_LOW, query, inView, bestIdx, bestDist, stats) == AMOS_OK ? 0 : -1;
}

}  // namespace ORB_SLAM2
