// pose_capi.cc -- C entry points that run Optimizer::PoseOptimization on a stand-in Frame: through the drop-in ORB_SLAM2::PoseOptimization
// (amos-slam_amd/host/FramePoseOptimization.h), or through amos_pose_core.h compiled for the host on one thread (the only host figure there
// is: g2o cannot be built without Eigen).  The stand-in Frame of tests/host/ref_standins.h has no SetPose; PoseFrame adds it.  Test
// harness: links the product library, never the other way round.
#include <chrono>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/amos_frontend.h"
#include "../host/ref_standins.h"
#include "../../amos-slam_amd/host/FramePoseOptimization.h"
#include "../../amos-slam_amd/csrc/amos_pose_core.h"

using namespace ORB_SLAM2;

namespace
{
struct PoseFrame : amos_standins::Frame {
    int nSetPose = 0;
    void SetPose(cv::Mat Tcw)  // Frame.cc:507-513 (UpdatePoseMatrices' products are the library's amos_pose_result.Ow)
    {
        mTcw = Tcw.clone();
        nSetPose++;
    }
};
thread_local std::string g_error;
}  // namespace

extern "C" {

const char *amos_host_pose_last_error(void) { return g_error.c_str(); }

// which = 0: ORB_SLAM2::PoseOptimization on a PoseFrame; 1: po::optimize_host on the same arrays.  camera: the start pose and intrinsics;
// has_point / world / obs: feature i's map point; outlier [n]: mvbOutlier, in and out.  `repeat` runs on fresh objects, the last one
// reported; ms = mean wall time of the call alone.  Out: Tcw [12] (rows of R | t), set_pose = calls of SetPose.  Returns the return value.
int amos_host_pose_optimization(const amos_pose_camera *camera, int n, const amos_keypoint *keys_un, const float *u_right, const uint8_t *has_point,
                                const float *world /* n x 3 */, const int32_t *obs, const float *inv_sigma2, int n_levels, int which, int repeat,
                                uint8_t *outlier, float *Tcw, int32_t *set_pose, double *ms)
{
    try {
        using namespace amos_standins;
        int result = 0;
        double total = 0;
        const int reps = repeat > 0 ? repeat : 1;
        std::vector<uint8_t> flags((size_t)n);
        for (int rep = 0; rep < reps; rep++) {
            PoseFrame F;
            F.N = n;
            F.mvKeysUn.resize(n);
            if (n) std::memcpy(F.mvKeysUn.data(), keys_un, sizeof(amos_keypoint) * n);
            F.mvKeys = F.mvKeysUn;
            if (u_right) F.mvuRight.assign(u_right, u_right + n);
            F.mvpMapPoints.assign(n, nullptr);
            F.mvbOutlier.assign(n, false);
            F.fx = camera->fx; F.fy = camera->fy; F.cx = camera->cx; F.cy = camera->cy; F.mbf = camera->mbf;
            F.mTcw = cv::Mat(4, 4, CV_32F);
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) F.mTcw.at<float>(r, c) = camera->Rcw[3 * r + c];
                F.mTcw.at<float>(r, 3) = camera->tcw[r];
                F.mTcw.at<float>(3, r) = 0.f;
            }
            F.mTcw.at<float>(3, 3) = 1.f;
            F.mnScaleLevels = n_levels;
            F.mvInvLevelSigma2.assign(inv_sigma2, inv_sigma2 + n_levels);
            std::vector<MapPoint> pts(n);
            for (int i = 0; i < n; i++) {
                F.mvbOutlier[i] = outlier[i] != 0;
                if (!has_point[i]) continue;
                for (int k = 0; k < 3; k++) pts[i].mWorldPos.at<float>(k, 0) = world[3 * i + k];
                pts[i].mnObs = obs[i];
                F.mvpMapPoints[i] = &pts[i];
            }
            if (which == 0) {
                const auto t0 = std::chrono::steady_clock::now();
                result = PoseOptimization<PoseFrame, MapPoint>(&F);
                total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (result < 0) { g_error = amos_last_error(); return -101; }
            } else {
                const auto t0 = std::chrono::steady_clock::now();
                std::vector<amos::po::Edge> edges;
                for (int i = 0; i < n; i++) {
                    if (!F.mvpMapPoints[i]) continue;
                    const cv::KeyPoint &kp = F.mvKeysUn[i];
                    if (kp.octave < 0 || kp.octave >= n_levels) continue;
                    const cv::Mat P = F.mvpMapPoints[i]->GetWorldPos();
                    edges.push_back(amos::po::Edge{kp.pt.x, kp.pt.y, u_right ? u_right[i] : -1.f, P.at<float>(0, 0), P.at<float>(1, 0), P.at<float>(2, 0),
                                                   inv_sigma2[kp.octave], i});
                }
                std::vector<unsigned char> out(edges.size() + 1, 0);
                amos::po::Out o;
                const amos::po::Cam cam{camera->fx, camera->fy, camera->cx, camera->cy, camera->mbf};
                result = amos::po::optimize_host(edges.data(), (int)edges.size(), out.data(), camera->Rcw, camera->tcw, cam, 0, o);
                if (edges.size() >= 3) {
                    for (size_t e = 0; e < edges.size(); e++) F.mvbOutlier[edges[e].feat] = out[e] != 0;
                    cv::Mat pose(4, 4, CV_32F);
                    for (int r = 0; r < 3; r++)
                        for (int c = 0; c < 4; c++) pose.at<float>(r, c) = o.Tcw[4 * r + c];
                    pose.at<float>(3, 0) = pose.at<float>(3, 1) = pose.at<float>(3, 2) = 0.f;
                    pose.at<float>(3, 3) = 1.f;
                    F.SetPose(pose);
                }
                total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
            if (rep + 1 < reps) continue;
            for (int i = 0; i < n; i++) flags[i] = F.mvbOutlier[i] ? 1 : 0;
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 4; c++) Tcw[4 * r + c] = F.mTcw.at<float>(r, c);
            *set_pose = F.nSetPose;
        }
        if (n) std::memcpy(outlier, flags.data(), (size_t)n);
        if (ms) *ms = total / reps;
        return result;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

}  // extern "C"
