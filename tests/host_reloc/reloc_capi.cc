// reloc_capi.cc -- C entry points that run the drop-ins of amos-slam_amd/host/FrameRelocalization.h on stand-in Frame / KeyFrame / MapPoint
// objects: ORB_SLAM2::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) and ORB_SLAM2::RefineRelocalization.  The stand-in
// Frame of tests/host/ref_standins.h has no SetPose; RelocFrame adds it.  Test harness: links the product library, never the other way round.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <set>
#include <string>
#include <vector>

#include "../../include/amos_host_types.h"
#include "../host/ref_standins.h"
#include "../../amos-slam_amd/host/FrameRelocalization.h"

using namespace ORB_SLAM2;

namespace
{
using namespace amos_standins;

struct RelocFrame : Frame {
    int nSetPose = 0;
    void SetPose(cv::Mat Tcw)  // Frame.cc:507-513
    {
        mTcw = Tcw.clone();
        nSetPose++;
    }
};
thread_local std::string g_error;
}  // namespace

extern "C" {

// the layouts of tests/host/host_capi.cc's amos_test_camera / amos_test_points / amos_test_kf
struct amos_reloc_test_camera {
    float fx, fy, cx, cy, mb, mbf;
    float min_x, max_x, min_y, max_y;
    float Tcw[16];
    int32_t n_levels;
    float scale_factors[AMOS_MAX_LEVELS];
};
struct amos_reloc_test_points {
    int32_t n;
    const float *world, *normal;
    const uint8_t *desc;
    const int32_t *obs;
    const uint8_t *bad;
    const float *min_dist, *max_dist;
};
struct amos_reloc_test_kf {
    amos_reloc_test_camera cam;
    int32_t n;
    const amos_keypoint *keys, *keys_un;
    const uint8_t *desc;
    const float *u_right;
    const int32_t *point_of;
    int32_t n_nodes;
    const uint32_t *node_ids;
    const int32_t *node_off, *node_idx;
};

}  // extern "C"

static std::vector<MapPoint> make_points(const amos_reloc_test_points *t)
{
    std::vector<MapPoint> pts(t->n);
    for (int i = 0; i < t->n; i++) {
        MapPoint &p = pts[i];
        for (int k = 0; k < 3; k++) p.mWorldPos.at<float>(k, 0) = t->world[3 * i + k];
        std::memcpy(p.mDescriptor.data, t->desc + 32 * (size_t)i, 32);
        p.mnObs = t->obs ? t->obs[i] : 1;
        p.mbBad = t->bad && t->bad[i];
        p.mfMinDistance = t->min_dist ? t->min_dist[i] : 0.f;
        p.mfMaxDistance = t->max_dist ? t->max_dist[i] : 1e9f;
    }
    return pts;
}

template <class F>
static void fill_base(F &f, const amos_reloc_test_kf *k, std::vector<MapPoint> &pts)
{
    const int n = k->n;
    f.N = n;
    f.mvKeys.resize(n);
    f.mvKeysUn.resize(n);
    if (n) {
        std::memcpy(f.mvKeys.data(), k->keys, sizeof(amos_keypoint) * n);
        std::memcpy(f.mvKeysUn.data(), k->keys_un, sizeof(amos_keypoint) * n);
    }
    f.mDescriptors = cv::Mat(std::max(n, 1), 32, CV_8U);
    if (n) std::memcpy(f.mDescriptors.data, k->desc, (size_t)32 * n);
    const amos_reloc_test_camera &c = k->cam;
    f.fx = c.fx; f.fy = c.fy; f.cx = c.cx; f.cy = c.cy; f.mb = c.mb; f.mbf = c.mbf;
    f.mnMinX = c.min_x; f.mnMaxX = c.max_x; f.mnMinY = c.min_y; f.mnMaxY = c.max_y;
    f.mnScaleLevels = c.n_levels;
    f.mvScaleFactors.assign(c.scale_factors, c.scale_factors + c.n_levels);
    f.mvInvLevelSigma2.resize(c.n_levels);
    for (int l = 0; l < c.n_levels; l++) f.mvInvLevelSigma2[l] = 1.0f / (c.scale_factors[l] * c.scale_factors[l]);  // ORBextractor.cc:522-533
    f.mfLogScaleFactor = c.n_levels > 1 ? std::log(c.scale_factors[1]) : 1.f;
    f.mvpMapPoints.assign(n, static_cast<MapPoint *>(NULL));
    for (int i = 0; i < n; i++)
        if (k->point_of && k->point_of[i] >= 0) f.mvpMapPoints[i] = &pts[k->point_of[i]];
}

static void fill_frame(RelocFrame &f, const amos_reloc_test_kf *k, std::vector<MapPoint> &pts)
{
    fill_base(f, k, pts);
    f.mvbOutlier.assign(k->n, false);
    f.mTcw = cv::Mat(4, 4, CV_32F);
    std::memcpy(f.mTcw.data, k->cam.Tcw, sizeof(float) * 16);
}

static inline int32_t index_of(const MapPoint *p, const std::vector<MapPoint> &pts) { return p ? (int32_t)(p - pts.data()) : -1; }

extern "C" {

const char *amos_host_reloc_last_error(void) { return g_error.c_str(); }

// ORB_SLAM2::SearchByProjection<Frame, KeyFrame, MapPoint>(CurrentFrame, pKF, sAlreadyFound, th, ORBdist, checkOri): the arguments of
// tests/host/host_capi.cc's amos_host_ref_search_reloc.  cur->point_of = the occupants of CurrentFrame.mvpMapPoints on entry;
// cur_points[i2] = CurrentFrame.mvpMapPoints[i2] on return (index into the point table or -1).  `repeat` runs on fresh objects, the last
// one reported; ms = mean wall time of the call alone.
int amos_host_reloc_search(const amos_reloc_test_kf *cur, const amos_reloc_test_kf *kf, const amos_reloc_test_points *points,
                           const uint8_t *already_found, float th, int orb_dist, int check_orientation, int repeat, int32_t *cur_points, double *ms)
{
    try {
        int n = 0;
        double total = 0;
        const int reps = repeat > 0 ? repeat : 1;
        for (int rep = 0; rep < reps; rep++) {
            std::vector<MapPoint> pts = make_points(points);
            RelocFrame Cur;
            KeyFrame KF;
            fill_frame(Cur, cur, pts);
            fill_base(KF, kf, pts);
            std::set<MapPoint *> found;
            for (int i = 0; i < points->n; i++)
                if (already_found && already_found[i]) found.insert(&pts[i]);
            const auto t0 = std::chrono::steady_clock::now();
            n = SearchByProjection<RelocFrame, KeyFrame, MapPoint>(Cur, &KF, found, th, orb_dist, check_orientation != 0);
            total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (n < 0) { g_error = amos_last_error(); return -101; }
            if (rep + 1 < reps) continue;
            for (int i = 0; i < cur->n; i++) cur_points[i] = index_of(Cur.mvpMapPoints[i], pts);
        }
        if (ms) *ms = total / reps;
        return n;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

// ORB_SLAM2::RefineRelocalization<Frame, KeyFrame, MapPoint>(CurrentFrame, pKF, vpMatches, vbInliers).  cur->cam.Tcw: the pose PnP found
// (what SetPose(Tcw) stored); vp_matches [cur->n]: index into the point table or -1 (vvpMapPointMatches[i]); inliers [cur->n].  Out:
// cur_points [cur->n] (mvpMapPoints), outlier [cur->n] (mvbOutlier), Tcw [12] (rows of R | t), set_pose = calls of SetPose.  Returns nGood.
int amos_host_refine_relocalization(const amos_reloc_test_kf *cur, const amos_reloc_test_kf *kf, const amos_reloc_test_points *points,
                                    const int32_t *vp_matches, const uint8_t *inliers, int32_t *cur_points, uint8_t *outlier, float *Tcw,
                                    int32_t *set_pose)
{
    try {
        std::vector<MapPoint> pts = make_points(points);
        RelocFrame Cur;
        KeyFrame KF;
        fill_frame(Cur, cur, pts);
        fill_base(KF, kf, pts);
        std::vector<MapPoint *> vpMatches(cur->n, static_cast<MapPoint *>(NULL));
        std::vector<bool> vbInliers(cur->n, false);
        for (int i = 0; i < cur->n; i++) {
            if (vp_matches[i] >= 0) vpMatches[i] = &pts[vp_matches[i]];
            vbInliers[i] = inliers[i] != 0;
        }
        const int nGood = RefineRelocalization<RelocFrame, KeyFrame, MapPoint>(Cur, &KF, vpMatches, vbInliers);
        if (nGood < 0) { g_error = amos_last_error(); return -101; }
        for (int i = 0; i < cur->n; i++) {
            cur_points[i] = index_of(Cur.mvpMapPoints[i], pts);
            outlier[i] = Cur.mvbOutlier[i] ? 1 : 0;
        }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) Tcw[4 * r + c] = Cur.mTcw.at<float>(r, c);
        *set_pose = Cur.nSetPose;
        return nGood;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

}  // extern "C"
