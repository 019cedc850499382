// KeyFrameSim3Search.h -- ORBmatcher::SearchBySim3 (ORBmatcher.cc:1314-1555) on the device: both directions and the agreement pass as ONE
// call of the C ABI (amos_match_sim3_search of include/amos_frontend.h: one upload, the grids of both keyframes, two launches, one download).
// The host keeps the pointer work: the map-point rows of the two keyframes, GetIndexInKeyFrame for the entries of vpMatches12, and the
// write-back of the accepted pairs.  The template gathers the arrays from the caller's KeyFrame / MapPoint objects.
#ifndef KEYFRAMESIM3SEARCH_H
#define KEYFRAMESIM3SEARCH_H

#include <cstring>
#include <vector>

#include "../../include/amos_host_types.h"
#include "FrameLocalPoints.h"     // LocalPointDistances
#include "ORBmatcher_adaptors.h"  // amos_adapt::pose_of, view_of
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The call itself on the calling thread's pooled matcher handle (FrameLocalPoints.h).  0, or -1 with the text in amos_last_error().
int SearchBySim3Views(const amos_frame_view &kf1, const amos_map_point *points1, const amos_frame_view &kf2, const amos_map_point *points2,
                      const amos_sim3_camera *cameras, const amos_sim3_search_pair &sim3, const float *scaleFactors, int nLevels,
                      const int32_t *match12, int32_t *matchOut, amos_sim3_search_stats *stats);

namespace amos_sim3_search
{
// GetMapPointMatches() by feature as the device reads it; a NULL or bad point carries the skip flag (the normal is not read)
template <class MapPointT>
inline void gather_points(const std::vector<MapPointT *> &vp, std::vector<amos_map_point> &points)
{
    points.resize(vp.size());
    for (size_t i = 0; i < vp.size(); i++) {
        amos_map_point &p = points[i];
        std::memset(&p, 0, sizeof(p));
        MapPointT *pMP = vp[i];
        if (!pMP || pMP->isBad()) {
            p.flags = AMOS_MAP_POINT_SKIP;
            continue;
        }
        const cv::Mat P = pMP->GetWorldPos(), d = pMP->GetDescriptor();
        for (int k = 0; k < 3; k++) p.pos[k] = P.template at<float>(k, 0);
        p.min_distance = LocalPointDistances<MapPointT>::Min(pMP);
        p.max_distance = LocalPointDistances<MapPointT>::Max(pMP);
        std::memcpy(p.desc, d.data, 32);
    }
}

template <class KeyFrameT>
inline amos_sim3_camera camera_of(KeyFrameT *pKF)
{
    const amos_adapt::Pose cw = amos_adapt::pose_of(pKF->GetRotation(), pKF->GetTranslation());
    amos_sim3_camera c;
    std::memcpy(c.Rcw, cw.R, sizeof(c.Rcw));
    std::memcpy(c.tcw, cw.t, sizeof(c.tcw));
    c.fx = pKF->fx; c.fy = pKF->fy; c.cx = pKF->cx; c.cy = pKF->cy;
    return c;
}
}  // namespace amos_sim3_search

// The reference's argument list and return value (LoopClosing.cc:454).  The level table and the image bounds are those the two keyframes
// share.  Returns nFound, or -1 when the library refused; then vpMatches12 is as it was.
template <class KeyFrameT, class MapPointT>
int SearchBySim3(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches12, const float &s12, const cv::Mat &R12, const cv::Mat &t12,
                 const float th)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    using namespace amos_adapt;
    const std::vector<MapPointT *> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    const int N1 = (int)vpMapPoints1.size(), N2 = (int)vpMapPoints2.size();
    std::vector<amos_map_point> points1, points2;
    amos_sim3_search::gather_points(vpMapPoints1, points1);
    amos_sim3_search::gather_points(vpMapPoints2, points2);
    std::vector<int32_t> row(N1 > 0 ? N1 : 1, -1), out(N1 > 0 ? N1 : 1, -1);
    for (int i = 0; i < N1; i++) {  // :1347-1357
        MapPointT *pMP = vpMatches12[i];
        if (!pMP) continue;
        const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
        row[i] = idx2 >= 0 && idx2 < N2 ? idx2 : AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE;
    }
    out = row;
    const amos_sim3_camera cams[2] = {amos_sim3_search::camera_of(pKF1), amos_sim3_search::camera_of(pKF2)};
    const Pose p12 = pose_of(R12, t12);
    amos_sim3_search_pair sim3;
    std::memcpy(sim3.R12, p12.R, sizeof(sim3.R12));
    std::memcpy(sim3.t12, p12.t, sizeof(sim3.t12));
    sim3.s12 = s12; sim3.th = th; sim3.enabled = 1;
    amos_frame_view v1 = view_of(*pKF1), v2 = view_of(*pKF2);
    v1.n = N1; v2.n = N2;
    amos_sim3_search_stats stats;
    if (SearchBySim3Views(v1, points1.data(), v2, points2.data(), cams, sim3, pKF1->mvScaleFactors.data(), (int)pKF1->mvScaleFactors.size(),
                          row.data(), out.data(), &stats) != 0) return -1;
    for (int i1 = 0; i1 < N1; i1++)  // :1539-1552
        if (out[i1] != row[i1] && out[i1] >= 0 && out[i1] < N2) vpMatches12[i1] = vpMapPoints2[out[i1]];
    return stats.n_found;
}

}  // namespace ORB_SLAM2

#endif
