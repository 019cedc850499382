// loop_points_capi.cc -- C entry points that build a stand-in keyframe and a list of stand-in map points from arrays and run
// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) on them through the drop-in (amos-slam_amd/host/KeyFrameLoopPoints.h) or
// through the host class (ORBmatcherFor, amos-slam_amd/host/ORBmatcher_adaptors.h), and the host compilation of
// amos-slam_amd/csrc/amos_loop_points_core.h.  Test harness: links the product library, never the other way round.
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/amos_host_types.h"
#include "../../amos-slam_amd/csrc/amos_loop_points_core.h"
#include "../../amos-slam_amd/host/ORBmatcher.h"
#include "../../amos-slam_amd/host/ORBmatcher_adaptors.h"
#include "../../amos-slam_amd/host/KeyFrameLoopPoints.h"

namespace lp_standins
{
class MapPoint
{
public:
    MapPoint() : mWorldPos(3, 1, CV_32F), mNormal(3, 1, CV_32F), mDescriptor(1, 32, CV_8U), mbBad(false), mfMinDistance(0.f), mfMaxDistance(1e9f) {}
    bool isBad() { return mbBad; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormal.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    template <class K> bool IsInKeyFrame(K *) { return false; }  // (the host class's shared pre-filter names it; this search does not ask)
    template <class F> int PredictScale(const float &currentDist, F *pF)
    {
        const float ratio = mfMaxDistance / currentDist;
        int nScale = (int)std::ceil(std::log(ratio) / pF->mfLogScaleFactor);
        if (nScale < 0) nScale = 0;
        else if (nScale >= pF->mnScaleLevels) nScale = pF->mnScaleLevels - 1;
        return nScale;
    }
    cv::Mat mWorldPos, mNormal, mDescriptor;
    bool mbBad;
    float mfMinDistance, mfMaxDistance;
};

class KeyFrame
{
public:
    bool IsInImage(const float &x, const float &y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    cv::Mat mDescriptors;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    int mnScaleLevels = 0;
    float mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
};
struct Frame {};  // (the host class's template wants a name; nothing of a Frame is used here)
}  // namespace lp_standins

using namespace lp_standins;

extern "C" {
struct amos_lp_kf {
    int32_t n;
    const amos_keypoint *keys_un;
    const uint8_t *desc;
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y;
    int32_t n_levels;
    float scale_factors[AMOS_MAX_LEVELS];
};
}

namespace
{
typedef ORB_SLAM2::ORBmatcherFor<Frame, KeyFrame, MapPoint> RefMatcher;
thread_local std::string g_error;

void build(KeyFrame &kf, const amos_lp_kf *k)
{
    const int n = k->n;
    kf.N = n;
    kf.mvKeysUn.resize(n);
    if (n) std::memcpy(kf.mvKeysUn.data(), k->keys_un, sizeof(amos_keypoint) * n);
    kf.mDescriptors = cv::Mat(n > 0 ? n : 1, 32, CV_8U);
    if (n) std::memcpy(kf.mDescriptors.data, k->desc, (size_t)32 * n);
    kf.fx = k->fx; kf.fy = k->fy; kf.cx = k->cx; kf.cy = k->cy;
    kf.mnMinX = k->min_x; kf.mnMaxX = k->max_x; kf.mnMinY = k->min_y; kf.mnMaxY = k->max_y;
    kf.mnScaleLevels = k->n_levels;
    kf.mfLogScaleFactor = std::log(k->scale_factors[1]);
    kf.mvScaleFactors.assign(k->scale_factors, k->scale_factors + k->n_levels);
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

extern "C" {

const char *amos_host_loop_points_last_error(void) { return g_error.c_str(); }

// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th).  points [n_points]: AMOS_MAP_POINT_SKIP = a point that isBad().  row_in [n]: vpMatched on
// entry: -1 = NULL, p >= 0 = the list's point p, -2 = a point that is not in the list.  row_out [n]: the same coding on return, -3 for a
// pointer that is none of these.  which = 0: the drop-in (stats: its record); 1: the host class.  `repeat` runs on fresh objects, the last one
// reported; ms[rep] is the wall time of the call alone.  -> nmatches
int amos_host_loop_points(const amos_lp_kf *k, const amos_map_point *points, int n_points, const float *Scw, const int32_t *row_in, int th, int which,
                          int repeat, int32_t *row_out, amos_loop_points_stats *stats, double *ms)
{
    try {
        int found = 0;
        for (int rep = 0; rep < (repeat > 1 ? repeat : 1); rep++) {
            KeyFrame kf;
            build(kf, k);
            std::vector<MapPoint> pts(n_points > 0 ? n_points : 1);
            std::vector<MapPoint *> vp(n_points, static_cast<MapPoint *>(NULL));
            for (int i = 0; i < n_points; i++) {
                MapPoint &mp = pts[i];
                const amos_map_point &p = points[i];
                for (int c = 0; c < 3; c++) {
                    mp.mWorldPos.at<float>(c, 0) = p.pos[c];
                    mp.mNormal.at<float>(c, 0) = p.normal[c];
                }
                std::memcpy(mp.mDescriptor.data, p.desc, 32);
                mp.mbBad = (p.flags & AMOS_MAP_POINT_SKIP) != 0;
                mp.mfMinDistance = p.min_distance;
                mp.mfMaxDistance = p.max_distance;
                vp[i] = &mp;
            }
            MapPoint elsewhere;
            std::vector<MapPoint *> vpMatched(k->n, static_cast<MapPoint *>(NULL));
            for (int i = 0; i < k->n; i++) {
                if (row_in[i] == -2) vpMatched[i] = &elsewhere;
                else if (row_in[i] >= 0) {
                    if (row_in[i] >= n_points) { g_error = "row_in names a point outside the list"; return -102; }
                    vpMatched[i] = &pts[row_in[i]];
                }
            }
            cv::Mat S(4, 4, CV_32F);
            std::memcpy(S.data, Scw, sizeof(float) * 16);
            const double t0 = now_ms();
            if (which == 0) {
                found = ORB_SLAM2::SearchByProjection(&kf, S, vp, vpMatched, th, stats);
            } else {
                RefMatcher matcher;
                found = matcher.SearchByProjection(&kf, S, vp, vpMatched, th);
            }
            if (ms) ms[rep] = now_ms() - t0;
            if (found < 0) { g_error = amos_last_error(); return -101; }
            for (int i = 0; i < k->n; i++) {
                MapPoint *p = vpMatched[i];
                row_out[i] = !p ? -1 : p == &elsewhere ? -2 : (p >= pts.data() && p < pts.data() + pts.size()) ? (int32_t)(p - pts.data()) : -3;
            }
        }
        return found;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

// The host compilation of amos_loop_points_core.h: out = Rcw [9], tcw [3], Ow [3], scw
void amos_host_loop_points_unscale(const float *Scw, float *out)
{
    amos::loop::Unscaled u;
    amos::loop::unscale(Scw, u);
    std::memcpy(out, u.Rcw, sizeof(float) * 9);
    std::memcpy(out + 9, u.tcw, sizeof(float) * 3);
    std::memcpy(out + 12, u.Ow, sizeof(float) * 3);
    out[15] = u.scw;
}

}  // extern "C"
