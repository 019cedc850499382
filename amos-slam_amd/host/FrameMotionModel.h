// FrameMotionModel.h -- the search of Tracking::TrackWithMotionModel (Tracking.cc:1925-1945) on the device: the fill of
// CurrentFrame.mvpMapPoints with NULL, ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1569-1728) and the
// second search with 2 * th when fewer than 20 matches came back, as ONE call of the C ABI (amos_match_motion_model of
// include/amos_frontend.h: one upload, the launches, one download).  The template gathers the arrays from the reference's objects and
// writes the result back; ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) itself is unchanged.
#ifndef FRAMEMOTIONMODEL_H
#define FRAMEMOTIONMODEL_H

#include <cstring>
#include <vector>

#include "../../include/amos_host_types.h"
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The call itself on a matcher handle that the calling thread owns (created on first use on amos_current_device(), or on AMOS_DEVICE).
// Returns the number of matches, or -1 with the text in amos_last_error().
int SearchByMotionModelArrays(const amos_keypoint *keysUn, const uint8_t *descriptors, const float *uRight, int N, const amos_last_point *points,
                              int nPoints, const amos_motion_camera &camera, const float *scaleFactors, int nLevels, float minX, float maxX,
                              float minY, float maxY, amos_proj_query *query, uint8_t *projected, int32_t *match, amos_motion_stats *stats);

// Replaces Tracking.cc:1925-1945: after mCurrentFrame.SetPose(mVelocity * mLastFrame.mTcw),
//     int nmatches = SearchByMotionModel<Frame, MapPoint>(mCurrentFrame, mLastFrame, th, mSensor == System::MONOCULAR);
// CurrentFrame.mvpMapPoints is overwritten as a whole (NULL where no point matched: the reference's fill is part of the call).  Returns the
// match count of the search whose result stands (-1: the library refused, nothing was written).
template <class FrameT, class MapPointT>
int SearchByMotionModel(FrameT &CurrentFrame, const FrameT &LastFrame, float th, bool bMono, bool checkOri = true)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    const int N = CurrentFrame.N, nPoints = LastFrame.N;
    std::vector<amos_last_point> points((size_t)nPoints);
    for (int i = 0; i < nPoints; i++) {
        amos_last_point &p = points[i];
        std::memset(&p, 0, sizeof(p));
        MapPointT *pMP = LastFrame.mvpMapPoints[i];
        if (!pMP || LastFrame.mvbOutlier[i]) {  // ORBmatcher.cc:1604-1608
            p.flags = AMOS_LAST_POINT_SKIP;
            continue;
        }
        const cv::Mat P = pMP->GetWorldPos(), d = pMP->GetDescriptor();
        for (int k = 0; k < 3; k++) p.pos[k] = P.template at<float>(k, 0);
        p.angle = LastFrame.mvKeysUn[i].angle;
        p.octave = LastFrame.mvKeys[i].octave;
        p.flags = pMP->Observations() > 0 ? AMOS_LAST_POINT_HAS_OBS : 0;
        std::memcpy(p.desc, d.data, 32);
    }
    amos_motion_camera cam;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            cam.Rcw[3 * r + c] = CurrentFrame.mTcw.template at<float>(r, c);
            cam.Rlw[3 * r + c] = LastFrame.mTcw.template at<float>(r, c);
        }
        cam.tcw[r] = CurrentFrame.mTcw.template at<float>(r, 3);
        cam.tlw[r] = LastFrame.mTcw.template at<float>(r, 3);
    }
    cam.fx = CurrentFrame.fx; cam.fy = CurrentFrame.fy; cam.cx = CurrentFrame.cx; cam.cy = CurrentFrame.cy;
    cam.mbf = CurrentFrame.mbf; cam.mb = CurrentFrame.mb;
    cam.th = th; cam.th_retry = 2 * th;  // Tracking.cc:1944
    cam.retry_below = 20;                // Tracking.cc:1941
    cam.mono = bMono; cam.check_orientation = checkOri;
    std::vector<uint8_t> desc((size_t)N * 32), projected((size_t)nPoints, 0);
    for (int i = 0; i < N; i++) std::memcpy(&desc[(size_t)i * 32], CurrentFrame.mDescriptors.ptr(i), 32);
    std::vector<amos_proj_query> query((size_t)nPoints);
    std::vector<int32_t> match((size_t)N, -1);
    amos_motion_stats stats;
    const bool stereo = (int)CurrentFrame.mvuRight.size() == N && N > 0;
    const int n = SearchByMotionModelArrays(reinterpret_cast<const amos_keypoint *>(CurrentFrame.mvKeysUn.data()), desc.data(),
                                            stereo ? CurrentFrame.mvuRight.data() : nullptr, N, points.data(), nPoints, cam,
                                            CurrentFrame.mvScaleFactors.data(), CurrentFrame.mnScaleLevels, CurrentFrame.mnMinX, CurrentFrame.mnMaxX,
                                            CurrentFrame.mnMinY, CurrentFrame.mnMaxY, query.data(), projected.data(), match.data(), &stats);
    if (n < 0) return n;
    for (int i = 0; i < N; i++) CurrentFrame.mvpMapPoints[i] = match[i] >= 0 ? LastFrame.mvpMapPoints[match[i]] : static_cast<MapPointT *>(NULL);
    return n;
}

}  // namespace ORB_SLAM2

#endif
