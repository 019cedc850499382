// sim3_optimize_capi.cc -- C entry points that build two stand-in keyframes with their map points and a stand-in Sim3 from arrays and run
// ORB_SLAM2::OptimizeSim3 (amos-slam_amd/host/KeyFrameSim3Optimize.h) on them, or run amos-slam_amd/csrc/amos_sim3_opt_core.h compiled for
// the host on one thread (the only host figure there is: g2o cannot be built without Eigen).  Test harness: links the product library,
// never the other way round.
#include <chrono>
#include <cstring>
#include <exception>
#include <map>
#include <string>
#include <vector>

#include "sim3_optimize_host.h"
#include "../../amos-slam_amd/host/KeyFrameSim3Optimize.h"

namespace s3o_standins
{
class KeyFrame;

class MapPoint
{
public:
    MapPoint() : mWorldPos(3, 1, CV_32F), mbBad(false) {}
    bool isBad() { return mbBad; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    int GetIndexInKeyFrame(KeyFrame *pKF)
    {
        std::map<KeyFrame *, size_t>::const_iterator it = mObservations.find(pKF);
        return it == mObservations.end() ? -1 : (int)it->second;
    }
    cv::Mat mWorldPos;
    bool mbBad;
    std::map<KeyFrame *, size_t> mObservations;
};

class KeyFrame
{
public:
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    cv::Mat GetRotation() { return cv::Mat(Tcw, cv::Rect(0, 0, 3, 3)).clone(); }
    cv::Mat GetTranslation() { return cv::Mat(Tcw, cv::Rect(3, 0, 1, 3)).clone(); }

    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat Tcw;
};

// g2o::Sim3's element access (sim3.h:239-264): r.coeffs() x, y, z, w, then t, then s
struct Sim3 {
    double v[8];
    double operator[](int i) const { return v[i]; }
    double &operator[](int i) { return v[i]; }
};
}  // namespace s3o_standins

using namespace s3o_standins;

extern "C" {
struct amos_s3o_kf {
    int32_t n;
    const amos_keypoint *keys_un;
    const amos_sim3_point *points;  // [n]: AMOS_SIM3_POINT_SKIP = no point at this feature; bit 2 of flags (value 4) = a point that isBad()
    amos_sim3_camera cam;
};
}

namespace
{
thread_local std::string g_error;

struct Standin {
    KeyFrame kf;
    std::vector<MapPoint> pts;
};

void build(Standin &s, const amos_s3o_kf *k, const float *inv_sigma2, int n_levels)
{
    KeyFrame &kf = s.kf;
    const int n = k->n;
    kf.mvKeysUn.resize(n);
    if (n) std::memcpy(kf.mvKeysUn.data(), k->keys_un, sizeof(amos_keypoint) * n);
    kf.mvInvLevelSigma2.assign(inv_sigma2, inv_sigma2 + n_levels);
    kf.fx = k->cam.fx; kf.fy = k->cam.fy; kf.cx = k->cam.cx; kf.cy = k->cam.cy;
    kf.Tcw = cv::Mat(4, 4, CV_32F);
    float T[16] = {0};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[4 * r + c] = k->cam.Rcw[3 * r + c];
        T[4 * r + 3] = k->cam.tcw[r];
    }
    T[15] = 1.f;
    std::memcpy(kf.Tcw.data, T, sizeof(T));
    s.pts = std::vector<MapPoint>(n > 0 ? n : 1);
    kf.mvpMapPoints.assign(n, static_cast<MapPoint *>(NULL));
    for (int i = 0; i < n; i++) {
        const amos_sim3_point &p = k->points[i];
        if ((p.flags & AMOS_SIM3_POINT_SKIP) && !(p.flags & 4)) continue;
        MapPoint &mp = s.pts[i];
        for (int c = 0; c < 3; c++) mp.mWorldPos.at<float>(c, 0) = p.pos[c];
        mp.mbBad = (p.flags & 4) != 0;
        mp.mObservations[&kf] = (size_t)i;
        kf.mvpMapPoints[i] = &mp;
    }
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

extern "C" {

const char *amos_host_sim3_optimize_last_error(void) { return g_error.c_str(); }

double amos_host_sim3_optimize_exp(double x) { return amos::so::exp_(x); }

// which = 0: ORB_SLAM2::OptimizeSim3 on stand-in objects.  row_in [n1]: -1 = NULL, j >= 0 = keyframe 2's point at feature j (it must
// exist), -2 = a point that is in neither keyframe.  The stand-in Sim3 is g2o::Sim3(R, t, s) of the pair's floats: r = Quaterniond(R).
// row_out [n1]: 1 where vpMatches1 is non-NULL on return, 0 where NULL.  sim3 [8]: the stand-in's elements on return.
// which = 1: the core on one host thread on the same arrays (any row_in); row_out [n1]: the row; result: the record; sim3 as the record has it.
// `repeat` runs on fresh objects, the last one reported; ms[rep] is the wall time of the call alone.  Returns the return value.
int amos_host_sim3_optimize(const amos_s3o_kf *kf1, const amos_s3o_kf *kf2, const int32_t *row_in, const amos_sim3_opt_pair *pair,
                            const float *inv_sigma2, int n_levels, int which, int repeat, int32_t *row_out, double *sim3,
                            amos_sim3_opt_result *result, double *ms)
{
    try {
        int ret = 0;
        for (int rep = 0; rep < (repeat > 1 ? repeat : 1); rep++) {
            if (which == 1) {
                const amos_sim3_camera cams[2] = {kf1->cam, kf2->cam};
                const double t0 = now_ms();
                ret = s3o_host::optimize(kf1->keys_un, kf1->points, kf1->n, kf2->keys_un, kf2->points, kf2->n, cams, row_in, inv_sigma2, n_levels,
                                         *pair, row_out, result);
                if (ms) ms[rep] = now_ms() - t0;
                for (int i = 0; i < 4; i++) sim3[i] = result->q[i];
                for (int i = 0; i < 3; i++) sim3[4 + i] = result->t[i];
                sim3[7] = result->s;
                continue;
            }
            Standin a, b;
            build(a, kf1, inv_sigma2, n_levels);
            build(b, kf2, inv_sigma2, n_levels);
            MapPoint elsewhere;
            std::vector<MapPoint *> vp(kf1->n, static_cast<MapPoint *>(NULL));
            for (int i = 0; i < kf1->n; i++) {
                if (row_in[i] == -2) vp[i] = &elsewhere;
                else if (row_in[i] >= 0) {
                    if (row_in[i] >= kf2->n || !b.kf.mvpMapPoints[row_in[i]]) { g_error = "row_in names a feature of keyframe 2 without a point"; return -102; }
                    vp[i] = b.kf.mvpMapPoints[row_in[i]];
                }
            }
            Sim3 S;
            double R[9];
            for (int i = 0; i < 9; i++) R[i] = (double)pair->R12[i];
            amos::po::quat_from_R(R, S.v);
            for (int i = 0; i < 3; i++) S.v[4 + i] = (double)pair->t12[i];
            S.v[7] = (double)pair->s12;
            const double t0 = now_ms();
            ret = ORB_SLAM2::OptimizeSim3(&a.kf, &b.kf, vp, S, pair->th2, pair->fix_scale != 0);
            if (ms) ms[rep] = now_ms() - t0;
            if (ret < 0) { g_error = amos_last_error(); return -101; }
            for (int i = 0; i < kf1->n; i++) row_out[i] = vp[i] ? 1 : 0;
            for (int i = 0; i < 8; i++) sim3[i] = S.v[i];
        }
        return ret;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

}  // extern "C"
