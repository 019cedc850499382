// KeyFrameFuse.h -- ORBmatcher::Fuse on the device: the pre-filter and the search of every map point (ORBmatcher.cc:1033-1148, :1199-1289)
// as ONE call of the C ABI for all target keyframes (amos_match_fuse of include/amos_frontend.h: one upload with every keyframe and the point
// list staged once, one launch, one download); the write-back (:1150-1170, :1291-1308: Replace / AddObservation / vpReplacePoint) stays on the
// host and runs in the reference's order.  The templates gather the arrays from the caller's KeyFrame / MapPoint objects.
#ifndef KEYFRAMEFUSE_H
#define KEYFRAMEFUSE_H

#include <chrono>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

#include "../../include/amos_host_types.h"
#include "FrameLocalPoints.h"     // LocalPointDistances
#include "ORBmatcher_adaptors.h"  // amos_adapt::pose_of, unscaled, centre, view_of; the view-based Fuse of the host class
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The call itself on the calling thread's pooled matcher handle (FrameLocalPoints.h).  0, or -1 with the text in amos_last_error().
int FuseViews(const amos_frame_view *kfs, int nKFs, const amos_map_point *points, int nPoints, int nPairs, const int32_t *pairFrame,
              const int32_t *pointFirst, const int32_t *pointCount, const int32_t *outOff, const amos_fuse_camera *cameras, const uint8_t *skip,
              int nOut, const float *scaleFactors, const float *invLevelSigma2, int nLevels, int mode, amos_window_query *query, uint8_t *inView,
              int32_t *bestIdx, int32_t *bestDist, amos_fuse_stats *stats);

// What a test or a profile may ask of FuseInNeighbors.
struct FuseTrace {
    int nHostSearches = 0;          // out: (point, keyframe) searches repeated on the host because the point's descriptor had changed
    double searchMs = 0;            // out: wall time of the device call and of the host re-searches (the rest of a call is gathering and write-back)
    bool keepStaleRecords = false;  // in: skip those repeats (WRONG results once a Replace of the call recomputed a descriptor: tests only)
};

namespace amos_fuse
{
// every list entry as the device reads it; a NULL or bad point carries the skip flag
template <class MapPointT>
inline void gather_points(const std::vector<MapPointT *> &vp, std::vector<amos_map_point> &points)
{
    points.resize(vp.size());
    for (size_t i = 0; i < vp.size(); i++) {
        amos_map_point &p = points[i];
        std::memset(&p, 0, sizeof(p));
        MapPointT *pMP = vp[i];
        if (!pMP || pMP->isBad()) {
            p.flags = AMOS_MAP_POINT_SKIP;
            continue;
        }
        const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal(), d = pMP->GetDescriptor();
        for (int k = 0; k < 3; k++) {
            p.pos[k] = P.template at<float>(k, 0);
            p.normal[k] = Pn.template at<float>(k, 0);
        }
        p.min_distance = LocalPointDistances<MapPointT>::Min(pMP);
        p.max_distance = LocalPointDistances<MapPointT>::Max(pMP);
        std::memcpy(p.desc, d.data, 32);
    }
}

template <class KeyFrameT>
inline amos_fuse_camera camera_of(KeyFrameT *pKF, const amos_adapt::Pose &cw, const amos_adapt::V3 &Ow, float th)
{
    amos_fuse_camera c;
    std::memcpy(c.Rcw, cw.R, sizeof(c.Rcw));
    std::memcpy(c.tcw, cw.t, sizeof(c.tcw));
    c.Ow[0] = Ow.x; c.Ow[1] = Ow.y; c.Ow[2] = Ow.z;
    c.fx = pKF->fx; c.fy = pKF->fy; c.cx = pKF->cx; c.cy = pKF->cy; c.mbf = pKF->mbf;
    c.th = th;
    return c;
}
}  // namespace amos_fuse

// Replaces the loop of LocalMapping::SearchInNeighbors over the target keyframes (LocalMapping.cc:673-682) around
//   matcher.Fuse(pKFi, vpMapPointMatches);
// with ONE device call over all targets; the write-backs then run keyframe by keyframe and point by point as the reference's loop does.
// Three things in that loop depend on an earlier write-back of the same call, and all three are honoured: a point made bad by an earlier
// Replace and a point that gained the keyframe through an earlier Replace / AddObservation are re-tested when the point's turn comes; and a
// point that SURVIVED a Replace has a new descriptor (MapPoint::Replace ends with ComputeDistinctiveDescriptors on the survivor,
// MapPoint.cc:303), so the reference searches it in the later targets with that descriptor.  Every point's descriptor is kept as it was
// gathered; from the first Replace of the call on, the points whose current descriptor differs from it are searched again on the host when a
// target's turn comes -- with the projection the device returned (u, v, ur and the level depend on position, normal and distance range,
// which nothing in Fuse changes) -- by the host class's view-based Fuse, one call per target; and a point's descriptor is compared once more
// when its own turn comes, and that one (point, keyframe) searched again on a one-entry list should it have changed in between.
// The level tables and the image bounds are those the targets share.  Returns the sum of nFused (*pnFused: per target), or -1 when the
// library refused; then nothing has been written back.
template <class KeyFrameT, class MapPointT>
int FuseInNeighbors(const std::vector<KeyFrameT *> &vpTargetKFs, const std::vector<MapPointT *> &vpMapPoints, const float th = 3.0,
                    std::vector<int> *pnFused = nullptr, FuseTrace *trace = nullptr)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    using namespace amos_adapt;
    const int nT = (int)vpTargetKFs.size(), nP = (int)vpMapPoints.size();
    if (pnFused) pnFused->assign(nT, 0);
    if (trace) trace->nHostSearches = 0, trace->searchMs = 0;
    if (nT == 0 || nP == 0) return 0;
    typedef std::chrono::steady_clock Clock;
    auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    std::vector<amos_map_point> points;
    amos_fuse::gather_points(vpMapPoints, points);
    std::vector<amos_frame_view> views(nT);
    std::vector<amos_fuse_camera> cams(nT);
    std::vector<int32_t> frame(nT), first(nT, 0), count(nT, nP), off(nT);
    std::vector<uint8_t> skip((size_t)nT * nP, 0);
    for (int k = 0; k < nT; k++) {
        KeyFrameT *pKF = vpTargetKFs[k];
        views[k] = view_of(*pKF);
        cams[k] = amos_fuse::camera_of(pKF, pose_of(pKF->GetRotation(), pKF->GetTranslation()), vec3(pKF->GetCameraCenter()), th);
        frame[k] = k;
        off[k] = k * nP;
        for (int i = 0; i < nP; i++) skip[(size_t)k * nP + i] = vpMapPoints[i] && vpMapPoints[i]->IsInKeyFrame(pKF);  // :1046
    }
    KeyFrameT *pKF0 = vpTargetKFs[0];
    const size_t nOut = (size_t)nT * nP;
    std::vector<amos_window_query> query(nOut);
    std::vector<uint8_t> inView(nOut, 0);
    std::vector<int32_t> bestIdx(nOut, -1), bestDist(nOut, 256);
    std::vector<amos_fuse_stats> stats(nT);
    const Clock::time_point tCall = Clock::now();
    if (FuseViews(views.data(), nT, points.data(), nP, nT, frame.data(), first.data(), count.data(), off.data(), cams.data(), skip.data(), (int)nOut,
                  pKF0->mvScaleFactors.data(), pKF0->mvInvLevelSigma2.data(), (int)pKF0->mvScaleFactors.size(), AMOS_FUSE_LOCAL, query.data(),
                  inView.data(), bestIdx.data(), bestDist.data(), stats.data()) != 0) return -1;
    if (trace) trace->searchMs += ms_since(tCall);
    bool replaced = false;  // a Replace of this call has run: descriptors may have changed
    std::unique_ptr<AMOS_VIEW_MATCHER> matcher;  // the host class for the repeats: one pooled handle, borrowed at the first repeat
    const bool repeat = !(trace && trace->keepStaleRecords);
    std::vector<uint8_t> searchedWith((size_t)nP * 32);  // the descriptor each record of the target at hand was searched with
    int total = 0;
    for (int k = 0; k < nT; k++) {
        KeyFrameT *pKF = vpTargetKFs[k];
        std::unique_ptr<FeatureGrid> grid;  // the host class's grid of this keyframe, built when the first repeat needs it
        auto search_again = [&](const std::vector<amos_window_query> &q, std::vector<int> &vnBestIdx) {
            const Clock::time_point t0 = Clock::now();
            if (!grid) grid.reset(new FeatureGrid(views[k]));
            if (!matcher) matcher.reset(new AMOS_VIEW_MATCHER());
            matcher->Fuse(*grid, q, pKF->mvScaleFactors, pKF->mvInvLevelSigma2, th, vnBestIdx);
            if (trace) trace->nHostSearches += (int)q.size(), trace->searchMs += ms_since(t0);
        };
        for (int i = 0; i < nP; i++) std::memcpy(&searchedWith[(size_t)i * 32], points[i].desc, 32);
        if (replaced && repeat) {
            // On entry of a target: every point whose descriptor is no longer the gathered one, in ONE call of the host class.  (A
            // descriptor that changes DURING this target's write-backs belongs to the survivor of a Replace in this keyframe, which the
            // filter below then skips; the comparison at a point's turn stays all the same, so nothing rests on that argument.)
            std::vector<amos_window_query> q;
            std::vector<int> at;
            for (int i = 0; i < nP; i++) {
                const size_t o = (size_t)k * nP + i;
                MapPointT *pMP = vpMapPoints[i];
                if (!pMP || !inView[o] || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
                const cv::Mat d = pMP->GetDescriptor();
                if (std::memcmp(d.data, points[i].desc, 32) == 0) continue;
                std::memcpy(&searchedWith[(size_t)i * 32], d.data, 32);
                q.push_back(query[o]);
                std::memcpy(q.back().desc, d.data, 32);
                at.push_back(i);
            }
            if (!q.empty()) {
                std::vector<int> vnBestIdx;
                search_again(q, vnBestIdx);
                for (size_t j = 0; j < at.size(); j++) bestIdx[(size_t)k * nP + at[j]] = vnBestIdx[j];
            }
        }
        int nFused = 0;
        for (int i = 0; i < nP; i++) {
            const size_t o = (size_t)k * nP + i;
            MapPointT *pMP = vpMapPoints[i];
            if (!pMP || !inView[o]) continue;
            if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;  // the reference's filter (:1046) when the point's turn comes
            int best = bestIdx[o];
            if (replaced && repeat) {
                const cv::Mat d = pMP->GetDescriptor();
                if (std::memcmp(d.data, &searchedWith[(size_t)i * 32], 32) != 0) {  // changed since the record was made: this one again
                    std::vector<amos_window_query> q(1, query[o]);
                    std::memcpy(q[0].desc, d.data, 32);
                    std::vector<int> vnBestIdx;
                    search_again(q, vnBestIdx);
                    best = vnBestIdx[0];
                }
            }
            if (best < 0) continue;
            MapPointT *pMPinKF = pKF->GetMapPoint(best);  // read now, as the reference does (:1150)
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations())
                        pMP->Replace(pMPinKF);
                    else
                        pMPinKF->Replace(pMP);
                    replaced = true;
                }
            } else {
                pMP->AddObservation(pKF, best);
                pKF->AddMapPoint(pMP, best);
            }
            nFused++;
        }
        if (pnFused) (*pnFused)[k] = nFused;
        total += nFused;
    }
    return total;
}

// The reference's argument list, ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:1020-1177): ONE pair on the device.  It serves the
// second call of LocalMapping::SearchInNeighbors (LocalMapping.cc:714), the current keyframe against the points of all targets.
template <class KeyFrameT, class MapPointT>
int Fuse(KeyFrameT *pKF, const std::vector<MapPointT *> &vpMapPoints, const float th = 3.0)
{
    return FuseInNeighbors(std::vector<KeyFrameT *>(1, pKF), vpMapPoints, th);
}

// ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1179-1312, LoopClosing::SearchAndFuse): ONE pair in AMOS_FUSE_SIM3
// mode, the points of spAlreadyFound (pKF->GetMapPoints() on entry, :1196) going in as skip bytes.  Nothing of this form changes a
// descriptor or makes a point bad under way.  Returns nFused (-1: the library refused, nothing written).
template <class KeyFrameT, class MapPointT>
int Fuse(KeyFrameT *pKF, cv::Mat Scw, const std::vector<MapPointT *> &vpPoints, float th, std::vector<MapPointT *> &vpReplacePoint)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    using namespace amos_adapt;
    const int nP = (int)vpPoints.size();
    if (nP == 0) return 0;
    const std::set<MapPointT *> spAlreadyFound = pKF->GetMapPoints();
    std::vector<amos_map_point> points;
    amos_fuse::gather_points(vpPoints, points);
    std::vector<uint8_t> skip(nP, 0);
    for (int i = 0; i < nP; i++) skip[i] = vpPoints[i] && spAlreadyFound.count(vpPoints[i]);  // :1208-1210
    const Pose cw = unscaled(Scw);
    const amos_frame_view view = view_of(*pKF);
    const amos_fuse_camera cam = amos_fuse::camera_of(pKF, cw, centre(cw), th);
    const int32_t zero = 0, n = nP;
    std::vector<amos_window_query> query(nP);
    std::vector<uint8_t> inView(nP, 0);
    std::vector<int32_t> bestIdx(nP, -1), bestDist(nP, 256);
    amos_fuse_stats stats;
    if (FuseViews(&view, 1, points.data(), nP, 1, &zero, &zero, &n, &zero, &cam, skip.data(), nP, pKF->mvScaleFactors.data(), nullptr,
                  (int)pKF->mvScaleFactors.size(), AMOS_FUSE_SIM3, query.data(), inView.data(), bestIdx.data(), bestDist.data(), &stats) != 0) return -1;
    int nFused = 0;
    for (int i = 0; i < nP; i++) {  // :1291-1308
        if (bestIdx[i] < 0) continue;
        MapPointT *pMP = vpPoints[i], *pMPinKF = pKF->GetMapPoint(bestIdx[i]);
        if (pMPinKF) {
            if (!pMPinKF->isBad()) vpReplacePoint[i] = pMPinKF;
        } else {
            pMP->AddObservation(pKF, bestIdx[i]);
            pKF->AddMapPoint(pMP, bestIdx[i]);
        }
        nFused++;
    }
    return nFused;
}

}  // namespace ORB_SLAM2

#endif
