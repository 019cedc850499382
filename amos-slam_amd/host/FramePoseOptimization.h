// FramePoseOptimization.h -- Optimizer::PoseOptimization(Frame *) (Optimizer.cc:363-605) on the device, as ONE call of the C ABI
// (amos_match_pose_optimization of include/amos_frontend.h: one upload, one launch, one download).  The template gathers the arrays from
// the reference's objects, writes mvbOutlier and calls pFrame->SetPose; its argument and return value are the reference's.  The arithmetic
// is amos-slam_amd/csrc/amos_pose_core.h (g2o's Levenberg-Marquardt restated; parity with a compiled g2o is not pinned).
#ifndef FRAMEPOSEOPTIMIZATION_H
#define FRAMEPOSEOPTIMIZATION_H

#include <vector>

#include "../../include/amos_frontend.h"
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The call itself on a matcher handle that the calling thread owns (created on first use on amos_current_device(), or on AMOS_DEVICE).
// Returns result->n_inliers, or -1 with the text in amos_last_error().
int PoseOptimizationArrays(const amos_keypoint *keysUn, const float *uRight, int N, int32_t *match, const float *pointsXyz, const uint8_t *hasObs,
                           int nPoints, const amos_pose_camera &camera, const float *invLevelSigma2, int nLevels, bool clearOutliers,
                           uint8_t *outlier, amos_pose_result *result);

// Replaces Optimizer::PoseOptimization(&mCurrentFrame) at Tracking.cc:1764, :1953, :2014 and inside Relocalization:
//     int nInliers = PoseOptimization<Frame, MapPoint>(&mCurrentFrame);
// Returns nInitialCorrespondences - nBad (-1: the library refused, nothing was written).  The discard loops behind the call sites read
// pFrame->mvbOutlier as before.
template <class FrameT, class MapPointT>
int PoseOptimization(FrameT *pFrame)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    const int N = pFrame->N;
    std::vector<int32_t> match((size_t)N, -1);
    std::vector<uint8_t> outlier((size_t)N, 0), hasObs;
    std::vector<float> xyz;
    for (int i = 0; i < N; i++) {
        MapPointT *pMP = pFrame->mvpMapPoints[i];
        outlier[i] = pFrame->mvbOutlier[i] ? 1 : 0;
        if (!pMP) continue;
        match[i] = (int32_t)hasObs.size();
        const cv::Mat P = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) xyz.push_back(P.template at<float>(k, 0));
        hasObs.push_back(pMP->Observations() > 0 ? 1 : 0);
    }
    amos_pose_camera cam;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cam.Rcw[3 * r + c] = pFrame->mTcw.template at<float>(r, c);
        cam.tcw[r] = pFrame->mTcw.template at<float>(r, 3);
    }
    cam.fx = pFrame->fx; cam.fy = pFrame->fy; cam.cx = pFrame->cx; cam.cy = pFrame->cy; cam.mbf = pFrame->mbf;
    const bool stereo = (int)pFrame->mvuRight.size() == N && N > 0;
    amos_pose_result res;
    const int n = PoseOptimizationArrays(reinterpret_cast<const amos_keypoint *>(pFrame->mvKeysUn.data()), stereo ? pFrame->mvuRight.data() : nullptr, N,
                                         match.data(), xyz.data(), hasObs.data(), (int)hasObs.size(), cam, pFrame->mvInvLevelSigma2.data(),
                                         (int)pFrame->mvInvLevelSigma2.size(), false, outlier.data(), &res);
    if (n < 0) return n;
    if (res.n_edges < 3) {  // Optimizer.cc:506: the flags of the matched features were reset on the way, the pose stays
        for (int i = 0; i < N; i++)
            if (match[i] >= 0) pFrame->mvbOutlier[i] = false;
        return 0;
    }
    for (int i = 0; i < N; i++) pFrame->mvbOutlier[i] = outlier[i] != 0;
    cv::Mat pose(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) pose.template at<float>(r, c) = res.Tcw[4 * r + c];
    pose.template at<float>(3, 0) = pose.template at<float>(3, 1) = pose.template at<float>(3, 2) = 0.f;
    pose.template at<float>(3, 3) = 1.f;
    pFrame->SetPose(pose);
    return n;
}

}  // namespace ORB_SLAM2

#endif
