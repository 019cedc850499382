// motion_capi.cc -- C entry point that runs the search of Tracking::TrackWithMotionModel (Tracking.cc:1925-1945) on stand-in Frame /
// MapPoint objects, either through the drop-in ORB_SLAM2::SearchByMotionModel (amos-slam_amd/host/FrameMotionModel.h) or through the chain
// the host classes had before it, written as Tracking writes it: fill, ORBmatcherFor::SearchByProjection(CurrentFrame, LastFrame, th, bMono),
// and below 20 matches fill and search again with 2 * th.  Test harness: links the product library, never the other way round.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/amos_host_types.h"
#include "../../amos-slam_amd/host/ORBmatcher.h"
#include "../../amos-slam_amd/host/ORBmatcher_adaptors.h"
#include "../host/ref_standins.h"
#include "../../amos-slam_amd/host/FrameMotionModel.h"

using namespace ORB_SLAM2;

namespace
{
typedef ORBmatcherFor<amos_standins::Frame, amos_standins::KeyFrame, amos_standins::MapPoint> RefMatcher;
thread_local std::string g_error;
}  // namespace

extern "C" {

struct amos_motion_test_camera {  // the layout of tests/host/host_capi.cc's amos_test_camera
    float fx, fy, cx, cy, mb, mbf;
    float min_x, max_x, min_y, max_y;
    float Tcw[16];
    int32_t n_levels;
    float scale_factors[AMOS_MAX_LEVELS];
};

static void fill_frame(amos_standins::Frame &F, const amos_motion_test_camera *cam, int n, const amos_keypoint *keys, const amos_keypoint *keys_un,
                       const uint8_t *desc, const float *u_right)
{
    F.N = n;
    F.mvKeys.resize(n);
    F.mvKeysUn.resize(n);
    if (n) {
        std::memcpy(F.mvKeys.data(), keys, sizeof(amos_keypoint) * n);
        std::memcpy(F.mvKeysUn.data(), keys_un, sizeof(amos_keypoint) * n);
    }
    F.mDescriptors = cv::Mat(std::max(n, 1), 32, CV_8U);
    if (n && desc) std::memcpy(F.mDescriptors.data, desc, (size_t)32 * n);
    if (u_right) F.mvuRight.assign(u_right, u_right + n);
    F.mvpMapPoints.assign(n, nullptr);
    F.mvbOutlier.assign(n, false);
    F.fx = cam->fx; F.fy = cam->fy; F.cx = cam->cx; F.cy = cam->cy; F.mb = cam->mb; F.mbf = cam->mbf;
    F.mnMinX = cam->min_x; F.mnMaxX = cam->max_x; F.mnMinY = cam->min_y; F.mnMaxY = cam->max_y;
    F.mTcw = cv::Mat(4, 4, CV_32F);
    std::memcpy(F.mTcw.data, cam->Tcw, sizeof(float) * 16);
    F.mnScaleLevels = cam->n_levels;
    F.mvScaleFactors.assign(cam->scale_factors, cam->scale_factors + cam->n_levels);
    F.mfLogScaleFactor = cam->n_levels > 1 ? std::log(cam->scale_factors[1]) : 1.f;
}

const char *amos_host_motion_last_error(void) { return g_error.c_str(); }

// which = 0: ORB_SLAM2::SearchByMotionModel; 1: the chain of Tracking.cc:1925-1945 over ORBmatcherFor::SearchByProjection.  Last frame: per
// feature has_point / outlier / world position / descriptor / observation count of its map point.  cur_junk[i2] (may be NULL): -1 =
// CurrentFrame.mvpMapPoints[i2] NULL on entry, else an occupant with that many observations sits there (both chains must clear it).
// `repeat` runs on fresh objects, the last one reported; ms = mean wall time of the chain alone.  Out: cur_match[i2] = index of the
// last-frame feature whose map point ends up in CurrentFrame.mvpMapPoints[i2], -1 for NULL, -2 for an occupant that survived.  Returns
// nmatches.
int amos_host_motion_model(const amos_motion_test_camera *cur_cam, int n_cur, const amos_keypoint *cur_keys_un, const uint8_t *cur_desc,
                           const float *cur_u_right, const int32_t *cur_junk, const amos_motion_test_camera *last_cam, int n_last,
                           const amos_keypoint *last_keys, const amos_keypoint *last_keys_un, const uint8_t *last_has_point,
                           const uint8_t *last_outlier, const float *last_world /* n x 3 */, const uint8_t *last_mp_desc /* n x 32 */,
                           const int32_t *last_mp_obs, float th, int mono, int which, int repeat, int32_t *cur_match, double *ms)
{
    try {
        using namespace amos_standins;
        int result = 0;
        double total = 0;
        const int reps = repeat > 0 ? repeat : 1;
        for (int rep = 0; rep < reps; rep++) {
            Frame Cur, Last;
            fill_frame(Cur, cur_cam, n_cur, cur_keys_un, cur_keys_un, cur_desc, cur_u_right);
            fill_frame(Last, last_cam, n_last, last_keys, last_keys_un, nullptr, nullptr);
            std::vector<MapPoint> pts(n_last), occupants(n_cur);
            for (int i = 0; i < n_last; i++) {
                if (!last_has_point[i]) continue;
                MapPoint &p = pts[i];
                for (int k = 0; k < 3; k++) p.mWorldPos.at<float>(k, 0) = last_world[3 * i + k];
                std::memcpy(p.mDescriptor.data, last_mp_desc + 32 * (size_t)i, 32);
                p.mnObs = last_mp_obs[i];
                Last.mvpMapPoints[i] = &p;
                Last.mvbOutlier[i] = last_outlier[i] != 0;
            }
            for (int i2 = 0; i2 < n_cur; i2++)
                if (cur_junk && cur_junk[i2] >= 0) {
                    occupants[i2].mnObs = cur_junk[i2];
                    Cur.mvpMapPoints[i2] = &occupants[i2];
                }
            const auto t0 = std::chrono::steady_clock::now();
            if (which == 0) {
                result = SearchByMotionModel<Frame, MapPoint>(Cur, Last, th, mono != 0);
                if (result < 0) { g_error = amos_last_error(); return -101; }
            } else {
                RefMatcher matcher(0.9, true);  // Tracking.cc:1910
                std::fill(Cur.mvpMapPoints.begin(), Cur.mvpMapPoints.end(), static_cast<MapPoint *>(NULL));
                result = matcher.SearchByProjection(Cur, Last, th, mono != 0);
                if (result < 20) {
                    std::fill(Cur.mvpMapPoints.begin(), Cur.mvpMapPoints.end(), static_cast<MapPoint *>(NULL));
                    result = matcher.SearchByProjection(Cur, Last, 2 * th, mono != 0);
                }
            }
            total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rep + 1 < reps) continue;
            for (int i2 = 0; i2 < n_cur; i2++) {
                const MapPoint *p = Cur.mvpMapPoints[i2];
                cur_match[i2] = !p ? -1 : (p >= pts.data() && p < pts.data() + n_last) ? (int32_t)(p - pts.data()) : -2;
            }
        }
        if (ms) *ms = total / reps;
        return result;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

}  // extern "C"
