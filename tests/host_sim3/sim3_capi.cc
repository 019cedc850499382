// sim3_capi.cc -- two things behind C entry points:
//   1. the HOST COMPILATION of the loop-closing Sim3 solver (sim3_host_solver.h over amos-slam_amd/csrc/amos_sim3_core.h).  The CPU tests
//      hold it to tests/sim3_restatement.py bit for bit, so the arithmetic the kernel shares is checked without a GPU;
//      tools/sim3_bench.py times it.
//   2. ORB_SLAM2::DeviceSim3Solver (amos-slam_amd/host/KeyFrameSim3.h) driven on stand-in KeyFrame / MapPoint objects: its host-side
//      constructor alone (no GPU), or the whole class over iterate() calls.
// Test harness: links the product library, never the other way round.
#include <chrono>
#include <exception>
#include <string>
#include <vector>

#include "sim3_host_solver.h"
#include "../host/ref_standins.h"
#include "../../amos-slam_amd/host/KeyFrameSim3.h"

using namespace ORB_SLAM2;

namespace
{
using namespace amos_standins;
thread_local std::string g_error;
}  // namespace

extern "C" {

const char *amos_host_sim3_last_error(void) { return g_error.c_str(); }

void *amos_host_sim3_solver_create(const amos_keypoint *kps1, const amos_sim3_point *points1, int n1, const amos_keypoint *kps2,
                                   const amos_sim3_point *points2, int n2, const amos_sim3_camera *cameras, const int32_t *match12,
                                   const float *level_sigma2, int n_levels, const amos_sim3_params *par)
{
    try {
        return new sim3_host::Solver(kps1, points1, n1, kps2, points2, n2, cameras, match12, level_sigma2, n_levels, *par);
    } catch (const std::exception &e) {
        g_error = e.what();
        return nullptr;
    }
}

void amos_host_sim3_solver_destroy(void *h) { delete static_cast<sim3_host::Solver *>(h); }

// Sim3Solver::iterate(n_iterations); inlier, match_out [n1] (match_out only with a Sim3); rng_state: the generator behind the call
int amos_host_sim3_solver_iterate(void *h, int n_iterations, amos_sim3_result *result, uint8_t *inlier, int32_t *match_out, uint64_t *rng_state)
{
    try {
        sim3_host::Solver &s = *static_cast<sim3_host::Solver *>(h);
        s.iterate(n_iterations, result, inlier, match_out);
        if (rng_state) *rng_state = s.rng;
        return 0;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

// the pieces on their own, for the CPU tests
int amos_host_sim3_parameters(int N, double probability, int min_inliers, int max_iterations)
{
    return amos::sim3::sim3_parameters(N, probability, min_inliers, max_iterations);
}

void amos_host_sim3_draw3(uint64_t *rng, int N, int32_t *idx)
{
    int out[3];
    amos::sim3::sim3_draw3(*rng, N, out);
    for (int k = 0; k < 3; k++) idx[k] = out[k];
}

// ORB_SLAM2::DeviceSim3Solver<KeyFrame, MapPoint> on stand-ins.  Keyframe k (k = 1, 2): keys [n_k], camera k - 1, a point table (world
// [np_k][3], bad [np_k], index_in_kf [np_k] = GetIndexInKeyFrame or -1) and kf_points [n_k] = the table index GetMapPointMatches() holds
// at the feature, or -1.  matched12 [n1] = index into table 2 or -1.  The constructor's arrays come back in keys1_out [n1], points1_out
// [n1], points2_out [n2], match12_out [n1].  With n_calls > 0: SetRansacParameters(probability, min_inliers, max_iterations), then
// n_calls times iterate(n_iterations); per call T12 [16] (zeros when empty), has_sim3, no_more, n_inliers, inliers [n1], and R [9], t [3],
// s of the getters.  ms: mean wall time of one iterate.  Returns 0.
int amos_host_sim3_dropin(const amos_keypoint *keys1, int n1, const amos_keypoint *keys2, int n2, const amos_sim3_camera *cameras,
                          const float *level_sigma2, int n_levels, const float *world1, const uint8_t *bad1, const int32_t *index1, int np1,
                          const int32_t *kf_points1, const float *world2, const uint8_t *bad2, const int32_t *index2, int np2,
                          const int32_t *kf_points2, const int32_t *matched12, int fix_scale, const uint64_t *seed, double probability,
                          int min_inliers, int max_iterations, int n_iterations, int n_calls, amos_keypoint *keys1_out,
                          amos_sim3_point *points1_out, amos_sim3_point *points2_out, int32_t *match12_out, float *T12, int32_t *has_sim3,
                          int32_t *no_more, int32_t *n_inliers, uint8_t *inliers, float *Rts, double *ms)
{
    try {
        KeyFrame kf[2];
        std::vector<MapPoint> pts[2] = {std::vector<MapPoint>((size_t)np1), std::vector<MapPoint>((size_t)np2)};
        const amos_keypoint *keys[2] = {keys1, keys2};
        const int n[2] = {n1, n2}, np[2] = {np1, np2};
        const float *world[2] = {world1, world2};
        const uint8_t *bad[2] = {bad1, bad2};
        const int32_t *index[2] = {index1, index2}, *kfPoints[2] = {kf_points1, kf_points2};
        for (int k = 0; k < 2; k++) {
            KeyFrame &K = kf[k];
            K.N = n[k];
            K.mvKeysUn.resize(n[k]);
            if (n[k]) std::memcpy(K.mvKeysUn.data(), keys[k], sizeof(amos_keypoint) * (size_t)n[k]);
            K.fx = cameras[k].fx; K.fy = cameras[k].fy; K.cx = cameras[k].cx; K.cy = cameras[k].cy;
            K.mnScaleLevels = n_levels;
            K.mvLevelSigma2.assign(level_sigma2, level_sigma2 + n_levels);
            K.Tcw = cv::Mat::zeros(4, 4, CV_32F);
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) K.Tcw.at<float>(r, c) = cameras[k].Rcw[3 * r + c];
                K.Tcw.at<float>(r, 3) = cameras[k].tcw[r];
            }
            K.Tcw.at<float>(3, 3) = 1.f;
            for (int i = 0; i < np[k]; i++) {
                for (int c = 0; c < 3; c++) pts[k][i].mWorldPos.at<float>(c, 0) = world[k][3 * i + c];
                pts[k][i].mbBad = bad[k][i] != 0;
                if (index[k][i] >= 0) pts[k][i].mObservations[&K] = (size_t)index[k][i];
            }
            K.mvpMapPoints.assign((size_t)n[k], static_cast<MapPoint *>(NULL));
            for (int i = 0; i < n[k]; i++)
                if (kfPoints[k][i] >= 0) K.mvpMapPoints[i] = &pts[k][kfPoints[k][i]];
        }
        std::vector<MapPoint *> vpMatched12((size_t)n1, static_cast<MapPoint *>(NULL));
        for (int i = 0; i < n1; i++)
            if (matched12[i] >= 0) vpMatched12[i] = &pts[1][matched12[i]];
        DeviceSim3Solver<KeyFrame, MapPoint> solver(&kf[0], &kf[1], vpMatched12, fix_scale != 0, *seed);
        if (n1) {
            std::memcpy(keys1_out, solver.Keys1().data(), sizeof(amos_keypoint) * (size_t)n1);
            std::memcpy(points1_out, solver.Points1().data(), sizeof(amos_sim3_point) * (size_t)n1);
            std::memcpy(match12_out, solver.Match12().data(), sizeof(int32_t) * (size_t)n1);
        }
        if (n2) std::memcpy(points2_out, solver.Points2().data(), sizeof(amos_sim3_point) * (size_t)n2);
        if (n_calls <= 0) return 0;
        solver.SetRansacParameters(probability, min_inliers, max_iterations);
        double total = 0;
        for (int call = 0; call < n_calls; call++) {
            bool bNoMore = false;
            std::vector<bool> vbInliers;
            int nInliers = 0;
            const auto t0 = std::chrono::steady_clock::now();
            cv::Mat T = solver.iterate(n_iterations, bNoMore, vbInliers, nInliers);
            total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (solver.Failed()) { g_error = amos_last_error(); return -101; }
            has_sim3[call] = T.empty() ? 0 : 1;
            no_more[call] = bNoMore ? 1 : 0;
            n_inliers[call] = nInliers;
            for (int k = 0; k < 16; k++) T12[16 * call + k] = T.empty() ? 0.f : T.at<float>(k / 4, k % 4);
            for (int i = 0; i < n1; i++) inliers[(size_t)call * n1 + i] = (i < (int)vbInliers.size() && vbInliers[i]) ? 1 : 0;
            const cv::Mat R = solver.GetEstimatedRotation(), t = solver.GetEstimatedTranslation();
            for (int k = 0; k < 9; k++) Rts[13 * call + k] = R.at<float>(k / 3, k % 3);
            for (int k = 0; k < 3; k++) Rts[13 * call + 9 + k] = t.at<float>(k, 0);
            Rts[13 * call + 12] = solver.GetEstimatedScale();
        }
        if (ms) *ms = total / n_calls;
        return 0;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

}  // extern "C"
