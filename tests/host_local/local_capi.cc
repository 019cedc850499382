// local_capi.cc -- C entry point that runs step 2 of Tracking::SearchLocalPoints on stand-in Frame / MapPoint objects, either through the
// drop-in ORB_SLAM2::SearchLocalPoints (amos-slam_amd/host/FrameLocalPoints.h) or through the chain the host classes had before it: the
// frustum test on the host, point by point, then ORBmatcherFor::SearchByProjection(F, vpMapPoints, th).  Test harness: links the product
// library, never the other way round.
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
#include "../../amos-slam_amd/host/FrameLocalPoints.h"

using namespace ORB_SLAM2;

namespace
{
// the members Tracking::SearchLocalPoints reads on top of the stand-ins of tests/host/ref_standins.h
struct LocalPoint : amos_standins::MapPoint {
    long unsigned int mnLastFrameSeen = 0;
    int mnVisible = 0;
    void IncreaseVisible(int n = 1) { mnVisible += n; }
};

struct LocalFrame : amos_standins::Frame {
    long unsigned int mnId = 1;
    cv::Mat mRcw, mtcw, mOw;

    // Frame::isInFrustum (Frame.cc:761-891) in the reference's order; the cv::Mat expressions as OpenCV evaluates them for CV_32F
    // (gemm and dot: double accumulation, one rounding; norm: double)
    bool isInFrustum(LocalPoint *pMP, float viewingCosLimit)
    {
        pMP->mbTrackInView = false;
        const cv::Mat P = pMP->GetWorldPos();
        float Pc[3], PO[3];
        for (int r = 0; r < 3; r++)
            Pc[r] = (float)((double)mRcw.at<float>(r, 0) * P.at<float>(0, 0) + (double)mRcw.at<float>(r, 1) * P.at<float>(1, 0) +
                            (double)mRcw.at<float>(r, 2) * P.at<float>(2, 0) + (double)mtcw.at<float>(r, 0));
        const float PcX = Pc[0], PcY = Pc[1], PcZ = Pc[2];
        if (PcZ < 0.0f) return false;
        const float invz = 1.0f / PcZ;
        const float u = fx * PcX * invz + cx;
        const float v = fy * PcY * invz + cy;
        if (u < mnMinX || u > mnMaxX) return false;
        if (v < mnMinY || v > mnMaxY) return false;
        const float maxDistance = pMP->GetMaxDistanceInvariance();
        const float minDistance = pMP->GetMinDistanceInvariance();
        double n2 = 0, dot = 0;
        const cv::Mat Pn = pMP->GetNormal();
        for (int r = 0; r < 3; r++) {
            PO[r] = P.at<float>(r, 0) - mOw.at<float>(r, 0);
            n2 += (double)PO[r] * PO[r];
            dot += (double)PO[r] * Pn.at<float>(r, 0);
        }
        const float dist = (float)std::sqrt(n2);
        if (dist < minDistance || dist > maxDistance) return false;
        const float viewCos = (float)(dot / dist);
        if (viewCos < viewingCosLimit) return false;
        const int nPredictedLevel = pMP->PredictScale(dist, this);
        pMP->mbTrackInView = true;
        pMP->mTrackProjX = u;
        pMP->mTrackProjXR = u - mbf * invz;
        pMP->mTrackProjY = v;
        pMP->mnTrackScaleLevel = nPredictedLevel;
        pMP->mTrackViewCos = viewCos;
        return true;
    }
};

typedef ORBmatcherFor<amos_standins::Frame, amos_standins::KeyFrame, amos_standins::MapPoint> RefMatcher;
thread_local std::string g_error;
}  // namespace

extern "C" {

struct amos_local_test_frame {
    float fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y;
    float Rcw[9], tcw[3], Ow[3];
    int32_t n_levels;
    float scale_factors[AMOS_MAX_LEVELS];
    int32_t n;
    const amos_keypoint *keys_un;
    const uint8_t *desc;
    const float *u_right;          // NULL: monocular
    const int32_t *occupant_obs;   // n: -1 = mvpMapPoints[i] NULL on entry, else the occupant's Observations()
};

struct amos_local_test_points {
    int32_t n;
    const float *world, *normal;   // n x 3
    const uint8_t *desc;           // n x 32
    const int32_t *obs;            // Observations()
    const uint8_t *bad, *seen;     // isBad(); mnLastFrameSeen == F.mnId
    const float *min_dist, *max_dist;
};

const char *amos_host_local_last_error(void) { return g_error.c_str(); }

// which = 0: ORB_SLAM2::SearchLocalPoints; 1: isInFrustum per point on the host, then ORBmatcherFor::SearchByProjection.  `repeat` runs on
// fresh objects, the last one reported; ms = mean wall time of the chain alone.  Out, per point: in_view (mbTrackInView), track
// [n x 4] = mTrackProjX, Y, XR, ViewCos, level, visible (IncreaseVisible calls); per feature: match = index of the point in mvpMapPoints[i],
// -1 NULL, -2 the untouched occupant.  Returns the match count.
int amos_host_local_points(const amos_local_test_frame *f, const amos_local_test_points *t, float th, float nnratio, int which, int repeat,
                           uint8_t *in_view, float *track, int32_t *level, int32_t *visible, int32_t *match, double *ms)
{
    try {
        int result = 0;
        double total = 0;
        for (int rep = 0; rep < (repeat > 0 ? repeat : 1); rep++) {
            LocalFrame F;
            F.N = f->n;
            F.mvKeysUn.resize(f->n);
            if (f->n) std::memcpy(F.mvKeysUn.data(), f->keys_un, sizeof(amos_keypoint) * f->n);
            F.mvKeys = F.mvKeysUn;
            F.mDescriptors = cv::Mat(std::max(f->n, 1), 32, CV_8U);
            if (f->n) std::memcpy(F.mDescriptors.data, f->desc, (size_t)32 * f->n);
            if (f->u_right) F.mvuRight.assign(f->u_right, f->u_right + f->n);
            F.mvbOutlier.assign(f->n, false);
            F.fx = f->fx; F.fy = f->fy; F.cx = f->cx; F.cy = f->cy; F.mbf = f->mbf; F.mb = f->mbf / f->fx;
            F.mnMinX = f->min_x; F.mnMaxX = f->max_x; F.mnMinY = f->min_y; F.mnMaxY = f->max_y;
            F.mRcw = cv::Mat(3, 3, CV_32F); F.mtcw = cv::Mat(3, 1, CV_32F); F.mOw = cv::Mat(3, 1, CV_32F);
            std::memcpy(F.mRcw.data, f->Rcw, sizeof(float) * 9);
            std::memcpy(F.mtcw.data, f->tcw, sizeof(float) * 3);
            std::memcpy(F.mOw.data, f->Ow, sizeof(float) * 3);
            F.mnScaleLevels = f->n_levels;
            F.mvScaleFactors.assign(f->scale_factors, f->scale_factors + f->n_levels);
            F.mfLogScaleFactor = f->n_levels > 1 ? std::log(f->scale_factors[1]) : 1.f;
            std::vector<LocalPoint> occupants(f->n), pts(t->n);
            F.mvpMapPoints.assign(f->n, nullptr);
            for (int i = 0; i < f->n; i++)
                if (f->occupant_obs && f->occupant_obs[i] >= 0) {
                    occupants[i].mnObs = f->occupant_obs[i];
                    F.mvpMapPoints[i] = &occupants[i];
                }
            std::vector<LocalPoint *> vp(t->n);
            std::vector<amos_standins::MapPoint *> vpBase(t->n);
            for (int i = 0; i < t->n; i++) {
                LocalPoint &p = pts[i];
                for (int k = 0; k < 3; k++) {
                    p.mWorldPos.at<float>(k, 0) = t->world[3 * i + k];
                    p.mNormal.at<float>(k, 0) = t->normal[3 * i + k];
                }
                std::memcpy(p.mDescriptor.data, t->desc + 32 * (size_t)i, 32);
                p.mnObs = t->obs[i];
                p.mbBad = t->bad[i] != 0;
                p.mnLastFrameSeen = t->seen[i] ? F.mnId : 0;
                p.mfMinDistance = t->min_dist[i];
                p.mfMaxDistance = t->max_dist[i];
                vp[i] = &p;
                vpBase[i] = &p;
            }
            const auto t0 = std::chrono::steady_clock::now();
            if (which == 0) {
                result = SearchLocalPoints(F, vp, th, nnratio);
                if (result < 0) { g_error = amos_last_error(); return -101; }
            } else {
                for (LocalPoint *pMP : vp) {  // Tracking.cc:2352-2372
                    if (pMP->mnLastFrameSeen == F.mnId) continue;
                    if (pMP->isBad()) continue;
                    if (F.isInFrustum(pMP, 0.5)) pMP->IncreaseVisible();
                }
                RefMatcher matcher(nnratio);
                result = matcher.SearchByProjection(F, vpBase, th);
            }
            total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rep + 1 < (repeat > 0 ? repeat : 1)) continue;
            for (int i = 0; i < t->n; i++) {
                in_view[i] = pts[i].mbTrackInView;
                track[4 * i] = pts[i].mTrackProjX; track[4 * i + 1] = pts[i].mTrackProjY;
                track[4 * i + 2] = pts[i].mTrackProjXR; track[4 * i + 3] = pts[i].mTrackViewCos;
                level[i] = pts[i].mnTrackScaleLevel;
                visible[i] = pts[i].mnVisible;
            }
            for (int i = 0; i < f->n; i++) {
                const amos_standins::MapPoint *p = F.mvpMapPoints[i];
                match[i] = !p ? -1 : (p >= pts.data() && p < pts.data() + t->n) ? (int32_t)(static_cast<const LocalPoint *>(p) - pts.data()) : -2;
            }
        }
        if (ms) *ms = total / (repeat > 0 ? repeat : 1);
        return result;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

}  // extern "C"
