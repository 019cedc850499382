// KeyFrameSearch.cc -- host side of ORB_SLAM2::SearchForTriangulation and SearchByBoW(pKF1, pKF2, ...): the calls of the C ABI on the calling
// thread's matcher handle; nothing of the searches is computed here.
#include "KeyFrameSearch.h"

#include "FrameLocalPoints.h"  // ThreadMatcherHandle

namespace ORB_SLAM2
{

int SearchForTriangulationViews(const amos_bow_view &k1, const amos_bow_view *const *k2s, int n2, const amos_kf_geometry *geometry,
                                const float *scaleFactors, const float *levelSigma2, int nLevels, bool onlyStereo, bool checkOri, int32_t *match12,
                                amos_bow_search_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    if (amos_match_triangulation(h, &k1, k2s, n2, geometry, scaleFactors, levelSigma2, nLevels, onlyStereo ? 1 : 0, checkOri ? 1 : 0, match12,
                                 stats) != AMOS_OK) return -1;
    int n = 0;
    for (int k = 0; k < n2; k++) n += stats[k].n_matches;
    return n;
}

int SearchByBoWKeyFrameViews(const amos_bow_view &k1, const amos_bow_view &k2, float nnratio, bool checkOri, int32_t *match12, amos_bow_search_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    if (amos_match_bow_kf(h, &k1, &k2, nnratio, checkOri ? 1 : 0, match12, stats) != AMOS_OK) return -1;
    return stats->n_matches;
}

}  // namespace ORB_SLAM2
