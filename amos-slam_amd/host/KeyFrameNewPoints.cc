// KeyFrameNewPoints.cc -- host side of ORB_SLAM2::CreateNewMapPointCandidates: the call of the C ABI on the calling thread's matcher handle;
// nothing of the search or the triangulation is computed here.
#include "KeyFrameNewPoints.h"

#include "FrameLocalPoints.h"  // ThreadMatcherHandle

namespace ORB_SLAM2
{

int CreateNewMapPointCandidatesViews(const amos_bow_view &k1, const amos_bow_view *const *k2s, int n2, const amos_kf_camera &cam1,
                                     const amos_kf_camera *cams2, const amos_keypoint *raw1, const amos_keypoint *const *raw2, const float *depth1,
                                     const float *const *depth2, const float *scaleFactors, const float *levelSigma2, int nLevels, bool checkOri,
                                     amos_new_point *newPoints, amos_new_points_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    if (amos_match_new_points(h, &k1, k2s, n2, &cam1, cams2, raw1, raw2, depth1, depth2, scaleFactors, levelSigma2, nLevels, 0, checkOri ? 1 : 0,
                              newPoints, stats) != AMOS_OK) return -1;
    int n = 0;
    for (int k = 0; k < n2; k++) n += stats[k].n_new;
    return n;
}

}  // namespace ORB_SLAM2
