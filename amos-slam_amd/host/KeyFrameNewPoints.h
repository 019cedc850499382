// KeyFrameNewPoints.h -- LocalMapping::CreateNewMapPoints (LocalMapping.cc:313-626) up to its `new MapPoint` as ONE call for all neighbours
// of the current keyframe (amos_match_new_points: geometry and baseline gate per neighbour, one upload with the current keyframe staged
// once, SearchForTriangulation's two launches and the triangulation's two, one download).  The template gathers the arrays from the
// caller's KeyFrame objects; what it returns per neighbour is the list the loop of :601-623 walks.  A keyframe-1 feature yields at most
// one candidate over all neighbours (the claim rule of include/amos_frontend.h, "new map points").
#ifndef KEYFRAMENEWPOINTS_H
#define KEYFRAMENEWPOINTS_H

#include <vector>

#include "../../include/amos_host_types.h"
#include "ORBmatcher_adaptors.h"  // amos_adapt::FlatFeatVec, bow_view_of, pose_of, vec3
#include "amos_cv.h"

namespace ORB_SLAM2
{

struct NewMapPointCandidate {
    size_t idx1, idx2;  // the feature in the current keyframe and in the neighbour
    float x3D[3];       // the world position `new MapPoint(x3D, ...)` takes
    int source;         // AMOS_NEW_POINT_TRIANGULATED / UNPROJECTED_1 / UNPROJECTED_2
};

// The call itself on the calling thread's pooled matcher handle (FrameLocalPoints.h).  Returns the number of candidates of all neighbours,
// or -1 with the text in amos_last_error().
int CreateNewMapPointCandidatesViews(const amos_bow_view &k1, const amos_bow_view *const *k2s, int n2, const amos_kf_camera &cam1,
                                     const amos_kf_camera *cams2, const amos_keypoint *raw1, const amos_keypoint *const *raw2, const float *depth1,
                                     const float *const *depth2, const float *scaleFactors, const float *levelSigma2, int nLevels, bool checkOri,
                                     amos_new_point *newPoints, amos_new_points_stats *stats);

namespace amos_adapt
{
template <class KeyFrameT>
inline amos_kf_camera kf_camera_of(KeyFrameT *pKF)
{
    amos_kf_camera c;
    const Pose p = pose_of(pKF->GetRotation(), pKF->GetTranslation());
    const V3 ow = vec3(pKF->GetCameraCenter());
    for (int i = 0; i < 9; i++) c.Rcw[i] = p.R[i];
    for (int i = 0; i < 3; i++) c.tcw[i] = p.t[i];
    c.Ow[0] = ow.x; c.Ow[1] = ow.y; c.Ow[2] = ow.z;
    c.fx = pKF->fx; c.fy = pKF->fy; c.cx = pKF->cx; c.cy = pKF->cy; c.invfx = pKF->invfx; c.invfy = pKF->invfy;
    c.mb = pKF->mb; c.mbf = pKF->mbf; c.scale_factor = pKF->mfScaleFactor;
    return c;
}
}  // namespace amos_adapt

// Replaces LocalMapping.cc:313-597: vvNew[k] gets the accepted matches of neighbour k in ascending idx1 -- the order in which the
// reference creates its MapPoints -- and what remains for the caller per entry e of vvNew[k] is :601-623:
//   MapPoint *pMP = new MapPoint(x3D of e, mpCurrentKeyFrame, mpMap); pMP->AddObservation(mpCurrentKeyFrame, e.idx1); ...
// A neighbour that fails the baseline gate (:361-374) gets an empty list.  The level tables are the current keyframe's (the keyframes of
// a map share one extractor's).  stats (optional): one record per neighbour.  Returns the number of candidates over all neighbours
// (-1: the library refused; every list is empty).
template <class KeyFrameT>
int CreateNewMapPointCandidates(KeyFrameT *pKF1, const std::vector<KeyFrameT *> &vpNeighKFs, std::vector<std::vector<NewMapPointCandidate> > &vvNew,
                                const bool checkOri = false, std::vector<amos_new_points_stats> *pStats = NULL)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    using namespace amos_adapt;
    const int n2 = (int)vpNeighKFs.size();
    vvNew.assign(n2, std::vector<NewMapPointCandidate>());
    if (pStats) pStats->assign(n2, amos_new_points_stats());
    if (n2 == 0) return 0;
    std::vector<std::vector<uint8_t> > has(n2 + 1);
    std::vector<FlatFeatVec> fvs;
    std::vector<amos_bow_view> views(n2 + 1);
    std::vector<amos_kf_camera> cams(n2 + 1);
    std::vector<const amos_keypoint *> raws(n2 + 1);
    std::vector<const float *> depths(n2 + 1);
    fvs.reserve(n2 + 1);
    for (int k = 0; k <= n2; k++) {
        KeyFrameT *pKF = k == 0 ? pKF1 : vpNeighKFs[k - 1];
        has[k].assign(pKF->N, 0);
        for (int i = 0; i < pKF->N; i++) has[k][i] = pKF->GetMapPoint(i) != NULL;  // ORBmatcher.cc:846-849, :874-877
        fvs.push_back(FlatFeatVec(pKF->mFeatVec));
        views[k] = bow_view_of(*pKF, pKF->mvKeysUn, fvs[k], &has[k], true);
        cams[k] = kf_camera_of(pKF);
        raws[k] = reinterpret_cast<const amos_keypoint *>(pKF->mvKeys.data());  // KeyFrame.cc:816-817
        depths[k] = pKF->mvDepth.empty() ? NULL : pKF->mvDepth.data();
    }
    std::vector<const amos_bow_view *> k2s(n2);
    for (int k = 0; k < n2; k++) k2s[k] = &views[k + 1];
    std::vector<amos_new_point> rows((size_t)n2 * (pKF1->N > 0 ? pKF1->N : 1));
    std::vector<amos_new_points_stats> stats(n2);
    const int n = CreateNewMapPointCandidatesViews(views[0], k2s.data(), n2, cams[0], cams.data() + 1, raws[0], raws.data() + 1, depths[0],
                                                   depths.data() + 1, pKF1->mvScaleFactors.data(), pKF1->mvLevelSigma2.data(),
                                                   (int)pKF1->mvScaleFactors.size(), checkOri, rows.data(), stats.data());
    if (n < 0) return n;
    for (int k = 0; k < n2; k++) {
        vvNew[k].resize(stats[k].n_new);
        for (int e = 0; e < stats[k].n_new; e++) {
            const amos_new_point &r = rows[(size_t)k * pKF1->N + e];
            NewMapPointCandidate &c = vvNew[k][e];
            c.idx1 = (size_t)r.idx1; c.idx2 = (size_t)r.idx2;
            c.x3D[0] = r.x; c.x3D[1] = r.y; c.x3D[2] = r.z;
            c.source = r.verdict;
        }
    }
    if (pStats) *pStats = stats;
    return n;
}

}  // namespace ORB_SLAM2

#endif
