// KeyFrameSearch.h -- the two searches over a pair of keyframes' FeatureVectors on the device: ORBmatcher::SearchForTriangulation
// (ORBmatcher.cc:810-1009), which LocalMapping::CreateNewMapPoints calls once per neighbour of the current keyframe, as ONE call for all
// neighbours (amos_match_triangulation: one upload with the current keyframe staged once, the two launches, one download), and
// ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (:656-799) of LoopClosing::ComputeSim3 (amos_match_bow_kf).  The templates gather the
// arrays from the caller's KeyFrame / MapPoint objects and write the results back; F12 and the poses stay the caller's.
#ifndef KEYFRAMESEARCH_H
#define KEYFRAMESEARCH_H

#include <utility>
#include <vector>

#include "../../include/amos_host_types.h"
#include "ORBmatcher_adaptors.h"  // amos_adapt::FlatFeatVec, bow_view_of, epipole_in
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The calls themselves on the calling thread's pooled matcher handle (FrameLocalPoints.h).  Return the number of matches (of all pairs), or
// -1 with the text in amos_last_error().
int SearchForTriangulationViews(const amos_bow_view &k1, const amos_bow_view *const *k2s, int n2, const amos_kf_geometry *geometry,
                                const float *scaleFactors, const float *levelSigma2, int nLevels, bool onlyStereo, bool checkOri, int32_t *match12,
                                amos_bow_search_stats *stats);
int SearchByBoWKeyFrameViews(const amos_bow_view &k1, const amos_bow_view &k2, float nnratio, bool checkOri, int32_t *match12, amos_bow_search_stats *stats);

// Replaces the loop of LocalMapping::CreateNewMapPoints over the neighbours (LocalMapping.cc:281-327) around
//   ORBmatcher matcher(0.6, false); matcher.SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, vMatchedIndices, false);
// with ONE call: vF12[k] is ComputeF12(pKF1, vpKF2s[k]) (3 x 3, CV_32F), vvMatchedPairs[k] gets the (idx1, idx2) pairs of neighbour k in
// ascending idx1.  The level tables are those of the first neighbour (the keyframes of a map share one extractor's).  Returns the number
// of matches over all neighbours (-1: the library refused; every vector is empty).
template <class KeyFrameT>
int SearchForTriangulation(KeyFrameT *pKF1, const std::vector<KeyFrameT *> &vpKF2s, const std::vector<cv::Mat> &vF12,
                           std::vector<std::vector<std::pair<size_t, size_t> > > &vvMatchedPairs, const bool bOnlyStereo, const bool checkOri = false)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    using namespace amos_adapt;
    const int n2 = (int)vpKF2s.size();
    vvMatchedPairs.assign(n2, std::vector<std::pair<size_t, size_t> >());
    if (n2 == 0) return 0;
    if ((int)vF12.size() != n2) return -1;
    std::vector<std::vector<uint8_t> > has(n2 + 1);
    std::vector<FlatFeatVec> fvs;
    std::vector<amos_bow_view> views(n2 + 1);
    std::vector<amos_kf_geometry> geo(n2);
    fvs.reserve(n2 + 1);
    for (int k = 0; k <= n2; k++) {
        KeyFrameT *pKF = k == 0 ? pKF1 : vpKF2s[k - 1];
        has[k].assign(pKF->N, 0);
        for (int i = 0; i < pKF->N; i++) has[k][i] = pKF->GetMapPoint(i) != NULL;  // :846-849, :874-877
        fvs.push_back(FlatFeatVec(pKF->mFeatVec));
        views[k] = bow_view_of(*pKF, pKF->mvKeysUn, fvs[k], &has[k], true);
        if (k == 0) continue;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) geo[k - 1].f12[3 * r + c] = vF12[k - 1].template at<float>(r, c);
        epipole_in(pKF1, pKF, geo[k - 1].ex, geo[k - 1].ey);
    }
    std::vector<const amos_bow_view *> k2s(n2);
    for (int k = 0; k < n2; k++) k2s[k] = &views[k + 1];
    std::vector<int32_t> match((size_t)n2 * pKF1->N, -1);
    std::vector<amos_bow_search_stats> stats(n2);
    KeyFrameT *first = vpKF2s[0];
    const int n = SearchForTriangulationViews(views[0], k2s.data(), n2, geo.data(), first->mvScaleFactors.data(), first->mvLevelSigma2.data(),
                                              (int)first->mvScaleFactors.size(), bOnlyStereo, checkOri, match.data(), stats.data());
    if (n < 0) return n;
    for (int k = 0; k < n2; k++) {  // :999-1006
        vvMatchedPairs[k].reserve(stats[k].n_matches);
        for (int i = 0; i < pKF1->N; i++)
            if (match[(size_t)k * pKF1->N + i] >= 0) vvMatchedPairs[k].push_back(std::make_pair((size_t)i, (size_t)match[(size_t)k * pKF1->N + i]));
    }
    return n;
}

// The reference's argument list: one neighbour.
template <class KeyFrameT>
int SearchForTriangulation(KeyFrameT *pKF1, KeyFrameT *pKF2, cv::Mat F12, std::vector<std::pair<size_t, size_t> > &vMatchedPairs, const bool bOnlyStereo,
                           const bool checkOri = false)
{
    std::vector<std::vector<std::pair<size_t, size_t> > > all;
    const int n = SearchForTriangulation(pKF1, std::vector<KeyFrameT *>(1, pKF2), std::vector<cv::Mat>(1, F12), all, bOnlyStereo, checkOri);
    vMatchedPairs.clear();
    if (n >= 0) vMatchedPairs.swap(all[0]);
    return n;
}

// Replaces ORBmatcher matcher(0.75, true); matcher.SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i]) (LoopClosing.cc:346): vpMatches12
// gets pKF1's map point count of entries, pKF2's map point where a feature matched and NULL elsewhere.  Returns the match count (-1: the
// library refused, vpMatches12 is all NULL).
template <class KeyFrameT, class MapPointT>
int SearchByBoW(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches12, float nnratio, bool checkOri)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    const std::vector<MapPointT *> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    vpMatches12 = std::vector<MapPointT *>(vpMapPoints1.size(), static_cast<MapPointT *>(NULL));
    std::vector<uint8_t> has1(pKF1->N, 0), has2(pKF2->N, 0);
    for (int i = 0; i < pKF1->N; i++) has1[i] = vpMapPoints1[i] && !vpMapPoints1[i]->isBad();  // :693-698
    for (int i = 0; i < pKF2->N; i++) has2[i] = vpMapPoints2[i] && !vpMapPoints2[i]->isBad();  // :710-716
    const amos_adapt::FlatFeatVec fv1(pKF1->mFeatVec), fv2(pKF2->mFeatVec);
    const amos_bow_view v1 = amos_adapt::bow_view_of(*pKF1, pKF1->mvKeysUn, fv1, &has1, false);
    const amos_bow_view v2 = amos_adapt::bow_view_of(*pKF2, pKF2->mvKeysUn, fv2, &has2, false);
    std::vector<int32_t> match((size_t)pKF1->N, -1);
    amos_bow_search_stats stats;
    const int n = SearchByBoWKeyFrameViews(v1, v2, nnratio, checkOri, match.data(), &stats);
    if (n < 0) return n;
    for (int i1 = 0; i1 < pKF1->N; i1++)
        if (match[i1] >= 0) vpMatches12[i1] = vpMapPoints2[match[i1]];
    return n;
}

}  // namespace ORB_SLAM2

#endif
