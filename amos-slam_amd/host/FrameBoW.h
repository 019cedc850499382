// FrameBoW.h -- the two steps of Tracking::TrackReferenceKeyFrame (Tracking.cc:1736-1794; Tracking::Relocalization runs the same two against
// every candidate keyframe) on the device: Frame::ComputeBoW (Frame.cc:1033-1049), i.e. DBoW2's TemplatedVocabulary::transform(features,
// BowVector&, FeatureVector&, 4), over a vocabulary tree that lives on the device (amos_bow_transform of include/amos_frontend.h), and
// ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:230-382) as ONE call of the C ABI (amos_match_bow: one upload, the two
// launches, one download).  The templates gather the arrays from the reference's objects and write the results back.
#ifndef FRAMEBOW_H
#define FRAMEBOW_H

#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/amos_host_types.h"
#include "ORBmatcher_adaptors.h"  // amos_adapt::FlatFeatVec, bow_view_of
#include "amos_cv.h"

namespace ORB_SLAM2
{

// ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) as far as tracking uses it: the text loader and the transform.
class DeviceVocabulary
{
public:
    DeviceVocabulary() {}
    ~DeviceVocabulary();
    DeviceVocabulary(const DeviceVocabulary &) = delete;
    DeviceVocabulary &operator=(const DeviceVocabulary &) = delete;

    // ORBvoc.txt's format (TemplatedVocabulary.h:1338-1424): a line "k L scoring weighting", then one line per node 1, 2, ...: parent id, leaf
    // flag, the descriptor's 32 bytes in decimal, the weight.  Host only: no device is touched.  Returns false, with status() ==
    // AMOS_ERR_INVALID and the text in error(), for a file that cannot be read, a line that does not parse (a missing or extra field, a
    // byte outside 0 .. 255) or a tree amos_bow_check refuses.  Empty lines are skipped (for a trailing one the reference appends a childless
    // inner node to the root, which a walk that chose it would leave the children array through).
    bool loadFromTextFile(const std::string &filename);
    bool empty() const { return parent_.size() < 2; }
    int status() const { return status_; }
    const std::string &error() const { return error_; }

    // what the file held; entry 0 of the node arrays is the root's and means nothing
    int k() const { return k_; }
    int L() const { return L_; }
    int scoring() const { return scoring_; }
    int weighting() const { return weighting_; }
    int nodes() const { return (int)parent_.size(); }
    int words() const { return nWords_; }
    const std::vector<int32_t> &parents() const { return parent_; }
    const std::vector<uint8_t> &leafFlags() const { return isLeaf_; }
    const std::vector<uint8_t> &descriptors() const { return desc_; }
    const std::vector<double> &weights() const { return weight_; }

    // TemplatedVocabulary::transform(features, v, fv, levelsup) (:1127-1194) on the device; n descriptors of 32 bytes.  The handle is created
    // on first use on amos_current_device(), or on AMOS_DEVICE; calls are serialised.  BowVec: a std::map<unsigned, double> (DBoW2::BowVector),
    // FeatVec: a std::map<unsigned, std::vector<unsigned>> (DBoW2::FeatureVector).  Returns AMOS_OK or the library's error (nothing is written).
    template <class BowVec, class FeatVec>
    int transform(const uint8_t *descriptors, int n, BowVec &v, FeatVec &fv, int levelsup)
    {
        Flat r;
        const int rc = transformArrays(descriptors, n, levelsup, r);
        if (rc != AMOS_OK) return rc;
        v.clear();
        fv.clear();
        for (int c = 0; c < r.stats.n_words; c++) v.insert(v.end(), typename BowVec::value_type(r.words[c], r.wordWeights[c]));
        for (int a = 0; a < r.stats.n_nodes; a++) {
            typename FeatVec::mapped_type &list = fv.insert(fv.end(), typename FeatVec::value_type(r.nodeIds[a], typename FeatVec::mapped_type()))->second;
            list.assign(r.nodeIdx.begin() + r.nodeOff[a], r.nodeIdx.begin() + r.nodeOff[a + 1]);
        }
        return AMOS_OK;
    }
    template <class BowVec, class FeatVec>
    int transform(const cv::Mat &descriptors, BowVec &v, FeatVec &fv, int levelsup)
    {
        return transform(descriptors.template ptr<unsigned char>(0), descriptors.rows, v, fv, levelsup);
    }

    struct Flat {  // amos_bow_transform's outputs
        std::vector<uint32_t> featWord, featNode, nodeIds, words;
        std::vector<int32_t> nodeOff, nodeIdx;
        std::vector<double> wordWeights;
        amos_bow_stats stats;
    };
    int transformArrays(const uint8_t *descriptors, int n, int levelsup, Flat &out);

private:
    int fail(const std::string &what);
    int k_ = 0, L_ = 0, scoring_ = 0, weighting_ = 0, nWords_ = 0, status_ = AMOS_OK;
    std::vector<int32_t> parent_;
    std::vector<uint8_t> isLeaf_, desc_;
    std::vector<double> weight_;
    std::string error_;
    std::mutex mutex_;
    amos_bow *handle_ = nullptr;
};

// Replaces Frame::ComputeBoW (Frame.cc:1033-1049):  ComputeBoW(mCurrentFrame, *mpDeviceVocabulary);  nothing is computed when mBowVec is
// already filled.  Returns AMOS_OK, or the library's error with both vectors untouched.
template <class FrameT>
int ComputeBoW(FrameT &F, DeviceVocabulary &voc, int levelsup = 4)
{
    if (!F.mBowVec.empty()) return AMOS_OK;
    return voc.transform(F.mDescriptors.template ptr<unsigned char>(0), F.N, F.mBowVec, F.mFeatVec, levelsup);
}

// The call itself on the calling thread's pooled matcher handle (FrameLocalPoints.h).  Returns the number of matches, or -1 with the text in
// amos_last_error().
int SearchByBoWViews(const amos_bow_view &kf, const amos_bow_view &f, float nnratio, bool checkOri, int32_t *matchesF, amos_bow_search_stats *stats);

// Replaces ORBmatcher matcher(nnratio, checkOri); matcher.SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:230-382; Tracking.cc:1745,
// :2634): vpMapPointMatches gets F.N entries, the keyframe's map point where a feature matched and NULL elsewhere.  Returns the match count
// (-1: the library refused, vpMapPointMatches is all NULL).
template <class KeyFrameT, class FrameT, class MapPointT>
int SearchByBoW(KeyFrameT *pKF, FrameT &F, std::vector<MapPointT *> &vpMapPointMatches, float nnratio, bool checkOri)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    const std::vector<MapPointT *> vpMapPointsKF = pKF->GetMapPointMatches();
    vpMapPointMatches = std::vector<MapPointT *>(F.N, static_cast<MapPointT *>(NULL));
    std::vector<uint8_t> has(pKF->N, 0);
    for (int i = 0; i < pKF->N; i++) has[i] = vpMapPointsKF[i] && !vpMapPointsKF[i]->isBad();  // :268-274
    const amos_adapt::FlatFeatVec fvKF(pKF->mFeatVec), fvF(F.mFeatVec);
    const amos_bow_view vKF = amos_adapt::bow_view_of(*pKF, pKF->mvKeysUn, fvKF, &has, false);
    const amos_bow_view vF = amos_adapt::bow_view_of(F, F.mvKeys, fvF, nullptr, false);  // :318 reads F.mvKeys[bestIdxF].angle
    std::vector<int32_t> match((size_t)F.N, -1);
    amos_bow_search_stats stats;
    const int n = SearchByBoWViews(vKF, vF, nnratio, checkOri, match.data(), &stats);
    if (n < 0) return n;
    for (int iF = 0; iF < F.N; iF++)
        if (match[iF] >= 0) vpMapPointMatches[iF] = vpMapPointsKF[match[iF]];
    return n;
}

}  // namespace ORB_SLAM2

#endif
