// FrameRelocalization.h -- steps 5 and 6 of Tracking::Relocalization's candidate loop (Tracking.cc:2700-2783) on the device:
// ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1731-1863) as ONE call of the C ABI
// (amos_match_reloc of include/amos_frontend.h: one upload, the launches, one download), and the refinement of one candidate composed of it
// and ORB_SLAM2::PoseOptimization (FramePoseOptimization.h).  The templates gather the arrays from the reference's objects and write the
// results back; ORBmatcher::SearchByProjection(Frame&, KeyFrame*, set, th, ORBdist) of the host class and its adaptor are unchanged.
#ifndef FRAMERELOCALIZATION_H
#define FRAMERELOCALIZATION_H

#include <cstring>
#include <set>
#include <vector>

#include "../../include/amos_host_types.h"
#include "FrameLocalPoints.h"  // LocalPointDistances: the raw mfMinDistance / mfMaxDistance of a MapPoint
#include "FramePoseOptimization.h"
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The call itself on the calling thread's matcher handle (ThreadMatcherHandle of FrameLocalPoints.h).  Returns nadditional, or -1 with the
// text in amos_last_error().
int SearchRelocalizationArrays(const amos_keypoint *keysUn, const uint8_t *descriptors, int N, const amos_reloc_point *points, int nPoints,
                               const uint8_t *found, const amos_reloc_camera &camera, const float *scaleFactors, int nLevels, float minX, float maxX,
                               float minY, float maxY, amos_kf_query *query, uint8_t *projected, int32_t *match, amos_reloc_stats *stats);

// Replaces matcher2.SearchByProjection(mCurrentFrame, vpCandidateKFs[i], sFound, th, ORBdist) at Tracking.cc:2732 and :2756:
//     int nadditional = SearchByProjection<Frame, KeyFrame, MapPoint>(mCurrentFrame, vpCandidateKFs[i], sFound, 10, 100);
// A keyframe feature is found when its MapPoint* is in sAlreadyFound, so a point that sits at two indices is found at both.  Only features
// whose mvpMapPoints entry is NULL on entry are written.  Returns nadditional (-1: the library refused, nothing was written).
template <class FrameT, class KeyFrameT, class MapPointT>
int SearchByProjection(FrameT &CurrentFrame, KeyFrameT *pKF, const std::set<MapPointT *> &sAlreadyFound, float th, int ORBdist, bool checkOri = true)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    const std::vector<MapPointT *> vpMPs = pKF->GetMapPointMatches();
    const int N = CurrentFrame.N, nPoints = (int)vpMPs.size();
    std::vector<amos_reloc_point> points((size_t)nPoints);
    std::vector<uint8_t> found((size_t)nPoints, 0);
    for (int i = 0; i < nPoints; i++) {
        amos_reloc_point &p = points[i];
        std::memset(&p, 0, sizeof(p));
        MapPointT *pMP = vpMPs[i];
        if (!pMP || pMP->isBad()) {  // ORBmatcher.cc:1752-1754
            p.flags = AMOS_RELOC_POINT_SKIP;
            continue;
        }
        found[i] = sAlreadyFound.count(pMP) ? 1 : 0;
        const cv::Mat P = pMP->GetWorldPos(), d = pMP->GetDescriptor();
        for (int k = 0; k < 3; k++) p.pos[k] = P.template at<float>(k, 0);
        p.angle = pKF->mvKeysUn[i].angle;
        p.min_distance = LocalPointDistances<MapPointT>::Min(pMP);
        p.max_distance = LocalPointDistances<MapPointT>::Max(pMP);
        p.flags = pMP->Observations() > 0 ? AMOS_RELOC_POINT_HAS_OBS : 0;
        std::memcpy(p.desc, d.data, 32);
    }
    amos_reloc_camera cam;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cam.Rcw[3 * r + c] = CurrentFrame.mTcw.template at<float>(r, c);
        cam.tcw[r] = CurrentFrame.mTcw.template at<float>(r, 3);
    }
    cam.fx = CurrentFrame.fx; cam.fy = CurrentFrame.fy; cam.cx = CurrentFrame.cx; cam.cy = CurrentFrame.cy;
    cam.th = th; cam.orb_dist = ORBdist; cam.check_orientation = checkOri;
    cam.found_from_match = 0;  // sAlreadyFound is the caller's: the PnP inliers at :2732, the frame's points at :2756
    cam.enabled = 1;
    std::vector<uint8_t> desc((size_t)N * 32), projected((size_t)nPoints, 0);
    std::vector<int32_t> match((size_t)N, -1);
    for (int i = 0; i < N; i++) {
        std::memcpy(&desc[(size_t)i * 32], CurrentFrame.mDescriptors.ptr(i), 32);
        if (CurrentFrame.mvpMapPoints[i]) match[i] = 0;  // set on entry (:1804); which point it is does not matter to the search
    }
    std::vector<amos_kf_query> query((size_t)nPoints);
    amos_reloc_stats stats;
    const int n = SearchRelocalizationArrays(reinterpret_cast<const amos_keypoint *>(CurrentFrame.mvKeysUn.data()), desc.data(), N, points.data(),
                                             nPoints, found.data(), cam, CurrentFrame.mvScaleFactors.data(), CurrentFrame.mnScaleLevels,
                                             CurrentFrame.mnMinX, CurrentFrame.mnMaxX, CurrentFrame.mnMinY, CurrentFrame.mnMaxY, query.data(),
                                             projected.data(), match.data(), &stats);
    if (n < 0) return n;
    for (int i = 0; i < N; i++)
        if (!CurrentFrame.mvpMapPoints[i] && match[i] >= 0) CurrentFrame.mvpMapPoints[i] = vpMPs[match[i]];  // :1820
    return n;
}

// Tracking.cc:2700-2783 for one candidate keyframe, after Tcw.copyTo(mCurrentFrame.mTcw) / SetPose(Tcw): the PnP inliers go into
// mvpMapPoints, PoseOptimization, and while the inliers stay below 50 the two projection searches (10, 100) and (3, 64) with an optimisation
// behind each.  PnPsolver, vbDiscarded and the choice of the candidate stay with the caller:
//     int nGood = RefineRelocalization<Frame, KeyFrame, MapPoint>(mCurrentFrame, vpCandidateKFs[i], vvpMapPointMatches[i], vbInliers);
//     if (nGood >= 50) { bMatch = true; break; }
// Returns nGood (-1: the library refused).
template <class FrameT, class KeyFrameT, class MapPointT>
int RefineRelocalization(FrameT &CurrentFrame, KeyFrameT *pKF, const std::vector<MapPointT *> &vpMatches, const std::vector<bool> &vbInliers)
{
    std::set<MapPointT *> sFound;
    const int np = (int)vbInliers.size();
    for (int j = 0; j < np; j++) {  // :2704-2713
        if (vbInliers[j]) {
            CurrentFrame.mvpMapPoints[j] = vpMatches[j];
            sFound.insert(vpMatches[j]);
        } else
            CurrentFrame.mvpMapPoints[j] = static_cast<MapPointT *>(NULL);
    }
    int nGood = PoseOptimization<FrameT, MapPointT>(&CurrentFrame);  // :2717
    if (nGood < 10) return nGood;
    for (int io = 0; io < CurrentFrame.N; io++)  // :2723-2725
        if (CurrentFrame.mvbOutlier[io]) CurrentFrame.mvpMapPoints[io] = static_cast<MapPointT *>(NULL);
    if (nGood < 50) {
        int nadditional = SearchByProjection<FrameT, KeyFrameT, MapPointT>(CurrentFrame, pKF, sFound, 10, 100);  // :2732
        if (nadditional < 0) return -1;
        if (nadditional + nGood >= 50) {
            nGood = PoseOptimization<FrameT, MapPointT>(&CurrentFrame);  // :2743 (no clearing loop behind it)
            if (nGood < 0) return -1;
            if (nGood > 30 && nGood < 50) {
                sFound.clear();  // :2752-2755
                for (int ip = 0; ip < CurrentFrame.N; ip++)
                    if (CurrentFrame.mvpMapPoints[ip]) sFound.insert(CurrentFrame.mvpMapPoints[ip]);
                nadditional = SearchByProjection<FrameT, KeyFrameT, MapPointT>(CurrentFrame, pKF, sFound, 3, 64);  // :2756
                if (nadditional < 0) return -1;
                if (nGood + nadditional >= 50) {
                    nGood = PoseOptimization<FrameT, MapPointT>(&CurrentFrame);  // :2766
                    if (nGood < 0) return -1;
                    for (int io = 0; io < CurrentFrame.N; io++)
                        if (CurrentFrame.mvbOutlier[io]) CurrentFrame.mvpMapPoints[io] = static_cast<MapPointT *>(NULL);
                }
            }
        }
    }
    return nGood;
}

}  // namespace ORB_SLAM2

#endif
