// KeyFrameSim3Search.cc -- host side of ORB_SLAM2::SearchBySim3: the call of the C ABI on the calling thread's matcher handle; nothing of
// the search is computed here.
#include "KeyFrameSim3Search.h"

namespace ORB_SLAM2
{

int SearchBySim3Views(const amos_frame_view &kf1, const amos_map_point *points1, const amos_frame_view &kf2, const amos_map_point *points2,
                      const amos_sim3_camera *cameras, const amos_sim3_search_pair &sim3, const float *scaleFactors, int nLevels,
                      const int32_t *match12, int32_t *matchOut, amos_sim3_search_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    return amos_match_sim3_search(h, &kf1, points1, &kf2, points2, cameras, &sim3, scaleFactors, nLevels, match12, matchOut, nullptr, nullptr,
                                  stats) == AMOS_OK ? 0 : -1;
}

}  // namespace ORB_SLAM2
