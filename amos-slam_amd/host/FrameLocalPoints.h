// FrameLocalPoints.h -- step 2 of Tracking::SearchLocalPoints (Tracking.cc:2352-2389) on the device: Frame::isInFrustum with
// MapPoint::PredictScale on every local map point, then ORBmatcher::SearchByProjection(F, vpMapPoints, th), as ONE call of the C ABI
// (amos_match_local_points of include/amos_frontend.h: one upload, the launches, one download).  The template gathers the arrays from the
// reference's objects and writes the results back; ORBmatcher::SearchByProjection(F, vpMapPoints, th) itself is unchanged.
#ifndef FRAMELOCALPOINTS_H
#define FRAMELOCALPOINTS_H

#include <cstring>
#include <vector>

#include "../../include/amos_host_types.h"
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The matcher handle that the calling thread owns (created on first use on amos_current_device(), or on AMOS_DEVICE; NULL with the text in
// amos_last_error() when that fails): the tracking thread's searches (this one, FrameMotionModel.h) share it.
amos_match *ThreadMatcherHandle();

// The call itself on the calling thread's handle.  Returns the number of matches, or -1 with the text in amos_last_error().
int SearchLocalPointsArrays(const amos_keypoint *keysUn, const uint8_t *descriptors, const float *uRight, int N, const amos_map_point *points,
                            int nPoints, const amos_local_camera &camera, const uint8_t *occupied, const float *scaleFactors, int nLevels,
                            float minX, float maxX, float minY, float maxY, amos_map_query *query, uint8_t *inView, int32_t *match,
                            amos_local_stats *stats);

// amos_map_point carries the RAW mfMinDistance / mfMaxDistance: PredictScale divides the raw maximum by the distance, and the 0.8f / 1.2f
// of GetMin / MaxDistanceInvariance are applied on the device.  The reference keeps the two members protected and exposes only the scaled
// values, so its MapPoint needs the two one-line accessors below (or a `friend`); specialise this for a class that names them otherwise.
template <class MapPointT>
struct LocalPointDistances {
    static float Min(MapPointT *p) { return p->mfMinDistance; }
    static float Max(MapPointT *p) { return p->mfMaxDistance; }
};

// Replaces the two loops' worth of Tracking.cc:2352-2389: every point that is neither bad nor already seen in this frame is tested;
// mbTrackInView is written on each of them, mTrackProjX / Y / XR, mnTrackScaleLevel and mTrackViewCos and IncreaseVisible() on those in
// view; F.mvpMapPoints[idx] receives the matched point.  Returns the match count (-1: the library refused, nothing was written).
template <class FrameT, class MapPointT>
int SearchLocalPoints(FrameT &F, const std::vector<MapPointT *> &vpLocalMapPoints, float th, float nnratio = 0.8f)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    const int N = F.N, nPoints = (int)vpLocalMapPoints.size();
    std::vector<amos_map_point> points((size_t)nPoints);
    for (int i = 0; i < nPoints; i++) {
        MapPointT *pMP = vpLocalMapPoints[i];
        amos_map_point &p = points[i];
        std::memset(&p, 0, sizeof(p));
        const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal(), d = pMP->GetDescriptor();
        for (int k = 0; k < 3; k++) {
            p.pos[k] = P.template at<float>(k, 0);
            p.normal[k] = Pn.template at<float>(k, 0);
        }
        p.min_distance = LocalPointDistances<MapPointT>::Min(pMP);
        p.max_distance = LocalPointDistances<MapPointT>::Max(pMP);
        p.flags = ((pMP->mnLastFrameSeen == F.mnId || pMP->isBad()) ? AMOS_MAP_POINT_SKIP : 0) | (pMP->Observations() > 0 ? AMOS_MAP_POINT_HAS_OBS : 0);
        std::memcpy(p.desc, d.data, 32);
    }
    amos_local_camera cam;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cam.Rcw[3 * r + c] = F.mRcw.template at<float>(r, c);
        cam.tcw[r] = F.mtcw.template at<float>(r, 0);
        cam.Ow[r] = F.mOw.template at<float>(r, 0);
    }
    cam.fx = F.fx; cam.fy = F.fy; cam.cx = F.cx; cam.cy = F.cy; cam.mbf = F.mbf;
    cam.view_cos_limit = 0.5f;  // Tracking.cc:2365
    cam.th = th; cam.nn_ratio = nnratio;
    std::vector<uint8_t> occupied((size_t)N, 0), desc((size_t)N * 32), inView((size_t)nPoints, 0);
    for (int i = 0; i < N; i++) {
        occupied[i] = F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0;  // ORBmatcher.cc:123-126
        std::memcpy(&desc[(size_t)i * 32], F.mDescriptors.ptr(i), 32);
    }
    std::vector<amos_map_query> query((size_t)nPoints);
    std::vector<int32_t> match((size_t)N, -1);
    amos_local_stats stats;
    const bool stereo = (int)F.mvuRight.size() == N && N > 0;
    const int n = SearchLocalPointsArrays(reinterpret_cast<const amos_keypoint *>(F.mvKeysUn.data()), desc.data(), stereo ? F.mvuRight.data() : nullptr, N,
                                          points.data(), nPoints, cam, occupied.data(), F.mvScaleFactors.data(), F.mnScaleLevels, F.mnMinX, F.mnMaxX,
                                          F.mnMinY, F.mnMaxY, query.data(), inView.data(), match.data(), &stats);
    if (n < 0) return n;
    for (int i = 0; i < nPoints; i++) {
        if (points[i].flags & AMOS_MAP_POINT_SKIP) continue;
        MapPointT *pMP = vpLocalMapPoints[i];
        pMP->mbTrackInView = inView[i] != 0;
        if (!inView[i]) continue;
        pMP->mTrackProjX = query[i].proj_x;
        pMP->mTrackProjXR = query[i].proj_xr;
        pMP->mTrackProjY = query[i].proj_y;
        pMP->mnTrackScaleLevel = query[i].level;
        pMP->mTrackViewCos = query[i].view_cos;
        pMP->IncreaseVisible();
    }
    for (int i = 0; i < N; i++)
        if (match[i] >= 0) F.mvpMapPoints[i] = vpLocalMapPoints[match[i]];  // ORBmatcher.cc:169
    return n;
}

}  // namespace ORB_SLAM2

#endif
