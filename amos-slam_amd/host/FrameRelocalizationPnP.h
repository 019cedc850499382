// FrameRelocalizationPnP.h -- step 3 of Tracking::Relocalization's candidate loop (Tracking.cc:2650-2713) on the device: ORB-SLAM2's
// PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) as a class with its constructor, SetRansacParameters and iterate, every iterate() ONE
// call of the C ABI (amos_match_reloc_pnp of include/amos_frontend.h: one upload, the launch, one download) on the calling thread's
// matcher handle.  The solver's carried state (generator, counters, best and refined sets) lives in a blob the object owns.
//     DevicePnPsolver<Frame, MapPoint> *pSolver = new DevicePnPsolver<Frame, MapPoint>(mCurrentFrame, vvpMapPointMatches[i]);
//     pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
//     cv::Mat Tcw = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
// The reference draws from the process-wide rand(); this class draws from one generator per solver, seeded by the constructor's third
// argument.  minSet other than 4 is refused (iterate returns an empty matrix with bNoMore set and Failed() true).
#ifndef FRAMERELOCALIZATIONPNP_H
#define FRAMERELOCALIZATIONPNP_H

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/amos_frontend.h"
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The call itself on the calling thread's matcher handle (ThreadMatcherHandle of FrameLocalPoints.h).  Returns 0, or -1 with the text in
// amos_last_error().
int RelocalizationPnPArrays(const amos_keypoint *keysUn, int N, const int32_t *bowMatch, const amos_reloc_point *points, int nPoints,
                            const float *levelSigma2, int nLevels, const amos_reloc_pnp_params &params, void *state, amos_reloc_pnp_result *result,
                            uint8_t *inlier, int32_t *match, uint8_t *found);
size_t RelocalizationPnPStateBytes(int N);

template <class FrameT, class MapPointT>
class DevicePnPsolver
{
public:
    // PnPsolver.cc:136-165: feature i is a correspondence when vpMapPointMatches[i] is a point that is not bad
    DevicePnPsolver(const FrameT &F, const std::vector<MapPointT *> &vpMapPointMatches, uint64_t seed = ~0ull)
        : mKeysUn(F.mvKeysUn.size()), mBowMatch(F.mvKeysUn.size(), -1), mPoints(vpMapPointMatches.size()), mLevelSigma2(F.mvLevelSigma2),
          mnMatches((int)vpMapPointMatches.size()), mbReset(true), mbFailed(false)
    {
        static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
        if (!mKeysUn.empty()) std::memcpy(mKeysUn.data(), F.mvKeysUn.data(), sizeof(amos_keypoint) * mKeysUn.size());
        for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
            amos_reloc_point &p = mPoints[i];
            std::memset(&p, 0, sizeof(p));
            MapPointT *pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) {
                p.flags = AMOS_RELOC_POINT_SKIP;
                continue;
            }
            const cv::Mat P = pMP->GetWorldPos();
            for (int k = 0; k < 3; k++) p.pos[k] = P.template at<float>(k, 0);
            if (i < mBowMatch.size()) mBowMatch[i] = (int32_t)i;
        }
        std::memset(&mParams, 0, sizeof(mParams));
        mParams.fx = F.fx; mParams.fy = F.fy; mParams.cx = F.cx; mParams.cy = F.cy;
        mParams.seed = seed;
        mParams.enabled = 1;
        std::memset(&mResult, 0, sizeof(mResult));
        mState.assign(RelocalizationPnPStateBytes((int)mKeysUn.size()), 0);
        SetRansacParameters();
    }

    // takes effect with the next iterate(), which starts the solver over (the reference sets its parameters once, before the first iterate)
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991)
    {
        mParams.probability = probability; mParams.min_inliers = minInliers; mParams.max_iterations = maxIterations;
        mParams.epsilon = epsilon; mParams.th2 = th2;
        mnMinSet = minSet;
        mbReset = true;
    }

    cv::Mat find(std::vector<bool> &vbInliers, int &nInliers)
    {
        bool bFlag;
        return iterate(mParams.max_iterations, bFlag, vbInliers, nInliers);
    }

    // PnPsolver.cc:240-363.  An empty matrix with bNoMore set and Failed() true: the library refused the call.
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        const int N = (int)mKeysUn.size();
        mParams.n_iterations = nIterations;
        mParams.reset = mbReset ? 1 : 0;
        std::vector<uint8_t> inlier((size_t)N, 0), found(mPoints.size(), 0);
        std::vector<int32_t> match((size_t)N, -1);
        mbFailed = mnMinSet != 4 || RelocalizationPnPArrays(mKeysUn.data(), N, mBowMatch.data(), mPoints.data(), (int)mPoints.size(), mLevelSigma2.data(),
                                                            (int)mLevelSigma2.size(), mParams, mState.data(), &mResult, inlier.data(), match.data(),
                                                            found.data()) != 0 || mResult.code != 0;
        if (mbFailed) {
            bNoMore = true;
            return cv::Mat();
        }
        mbReset = false;
        bNoMore = mResult.no_more != 0;
        if (!mResult.has_pose) return cv::Mat();
        nInliers = mResult.n_inliers;
        vbInliers.assign((size_t)mnMatches, false);  // vector<bool>(mvpMapPointMatches.size(), false)
        for (int i = 0; i < N && i < mnMatches; i++) vbInliers[i] = inlier[i] != 0;
        cv::Mat Tcw = cv::Mat::zeros(4, 4, CV_32F);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) Tcw.at<float>(r, c) = mResult.Tcw[4 * r + c];
        Tcw.at<float>(3, 3) = 1.f;
        return Tcw;
    }

    bool Failed() const { return mbFailed; }
    const amos_reloc_pnp_result &LastResult() const { return mResult; }

private:
    std::vector<amos_keypoint> mKeysUn;
    std::vector<int32_t> mBowMatch;
    std::vector<amos_reloc_point> mPoints;
    std::vector<float> mLevelSigma2;
    std::vector<uint8_t> mState;
    amos_reloc_pnp_params mParams;
    amos_reloc_pnp_result mResult;
    int mnMatches, mnMinSet;
    bool mbReset, mbFailed;
};

}  // namespace ORB_SLAM2

#endif
