// KeyFrameLoopPoints.h -- ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:388-512, the last search of
// LoopClosing::ComputeSim3) on the device: Scw's decomposition, the pre-filter and the greedy search as ONE call of the C ABI
// (amos_match_loop_points of include/amos_frontend.h: one upload, the keyframe's grid, the launches, one download).  The host keeps the
// pointer work: spAlreadyFound as one byte per point, vpMatched as a row of occupied features, and vpMatched[bestIdx] = pMP.  The template
// gathers the arrays from the caller's KeyFrame / MapPoint objects.
#ifndef KEYFRAMELOOPPOINTS_H
#define KEYFRAMELOOPPOINTS_H

#include <cstring>
#include <set>
#include <vector>

#include "../../include/amos_host_types.h"
#include "KeyFrameFuse.h"         // amos_fuse::gather_points
#include "ORBmatcher_adaptors.h"  // amos_adapt::view_of
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The call itself on the calling thread's pooled matcher handle (FrameLocalPoints.h).  0, or -1 with the text in amos_last_error().
int SearchLoopPointsView(const amos_frame_view &kf, const amos_map_point *points, int nPoints, const amos_loop_points_query &query,
                         const int32_t *matched, const uint8_t *found, const float *scaleFactors, int nLevels, int32_t *loopMatch,
                         amos_loop_points_stats *stats);

// The reference's argument list and return value (LoopClosing.cc:534).  Returns nmatches, or -1 when the library refused; then vpMatched
// is as it was.  pStats (optional): the call's record, n_total and accepted at min_total = 40 among it.
template <class KeyFrameT, class MapPointT>
int SearchByProjection(KeyFrameT *pKF, cv::Mat Scw, const std::vector<MapPointT *> &vpPoints, std::vector<MapPointT *> &vpMatched, int th,
                       amos_loop_points_stats *pStats = nullptr)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    const int nP = (int)vpPoints.size();
    amos_frame_view view = amos_adapt::view_of(*pKF);
    const int N = view.n;
    std::set<MapPointT *> spAlreadyFound(vpMatched.begin(), vpMatched.end());  // :407-408
    spAlreadyFound.erase(static_cast<MapPointT *>(NULL));
    std::vector<amos_map_point> points;
    amos_fuse::gather_points(vpPoints, points);
    std::vector<uint8_t> found(nP > 0 ? nP : 1, 0);
    for (int i = 0; i < nP; i++) found[i] = vpPoints[i] && spAlreadyFound.count(vpPoints[i]);  // :420
    std::vector<int32_t> row(N > 0 ? N : 1, -1), out(N > 0 ? N : 1, -1);
    for (int i = 0; i < N && i < (int)vpMatched.size(); i++)
        if (vpMatched[i]) row[i] = AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE;  // :482: any non-NULL entry occupies the feature
    amos_loop_points_query q;
    std::memset(&q, 0, sizeof(q));
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) q.Scw[4 * r + c] = Scw.template at<float>(r, c);
    q.fx = pKF->fx; q.fy = pKF->fy; q.cx = pKF->cx; q.cy = pKF->cy;
    q.th = (float)th;
    q.frame = 0; q.max_dist = AMOS_TH_LOW; q.min_inliers = 20; q.min_total = 40; q.enabled = 1; q.found_from_match = 0;
    amos_loop_points_stats stats;
    if (SearchLoopPointsView(view, points.data(), nP, q, row.data(), found.data(), pKF->mvScaleFactors.data(), (int)pKF->mvScaleFactors.size(),
                             out.data(), &stats) != 0) return -1;
    for (int i = 0; i < N && i < (int)vpMatched.size(); i++)
        if (out[i] >= 0 && out[i] < nP) vpMatched[i] = vpPoints[out[i]];  // :500
    if (pStats) *pStats = stats;
    return stats.n_matches;
}

}  // namespace ORB_SLAM2

#endif
