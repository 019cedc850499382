// KeyFrameSim3.h -- step 2 of LoopClosing::ComputeSim3's candidate loop (LoopClosing.cc:389-447) on the device: ORB-SLAM2's Sim3Solver
// (include/Sim3Solver.h, src/Sim3Solver.cc) as a class with its constructor, SetRansacParameters, iterate, find and the three getters,
// every iterate() ONE call of the C ABI (amos_match_sim3 of include/amos_frontend.h: one upload, the launch, one download) on the calling
// thread's matcher handle.  The solver's carried state (generator, counters, best Sim3 and inlier set) lives in a blob the object owns.
//     DeviceSim3Solver<KeyFrame, MapPoint> *pSolver = new DeviceSim3Solver<KeyFrame, MapPoint>(mpCurrentKF, pKF, vvpMapPointMatches[i], mbFixScale);
//     pSolver->SetRansacParameters(0.99, 20, 300);
//     cv::Mat Scm = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
// The constructor does the pointer work of Sim3Solver.cc:78-127 on the host: feature i1 is a correspondence when vpMatched12[i1] and
// pKF1's own point at i1 are good points with an index in their keyframes; the point positions go into per-feature records and the
// match row holds indexKF2.  A feature whose indexKF1 is not i1 gets that keypoint's octave in the solver's own copy of the keypoint row.
// The reference draws from the process-wide rand(); this class draws from one generator per solver, seeded by the constructor's last
// argument.  minInliers below 3 is refused by the library (iterate returns an empty matrix with bNoMore set and Failed() true).
#ifndef KEYFRAMESIM3_H
#define KEYFRAMESIM3_H

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/amos_frontend.h"
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The call itself on the calling thread's matcher handle (ThreadMatcherHandle of FrameLocalPoints.h).  Returns 0, or -1 with the text in
// amos_last_error().
int Sim3Arrays(const amos_keypoint *keys1, const amos_sim3_point *points1, int n1, const amos_keypoint *keys2, const amos_sim3_point *points2, int n2,
               const amos_sim3_camera *cameras, const int32_t *match12, const float *levelSigma2, int nLevels, const amos_sim3_params &params,
               void *state, amos_sim3_result *result, uint8_t *inlier, int32_t *matchOut);
size_t Sim3StateBytes(int n1);

template <class KeyFrameT, class MapPointT>
class DeviceSim3Solver
{
public:
    DeviceSim3Solver(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<MapPointT *> &vpMatched12, const bool bFixScale, uint64_t seed = ~0ull)
        : mKeys1(pKF1->mvKeysUn.size()), mKeys2(pKF2->mvKeysUn.size()), mPoints1(pKF1->mvKeysUn.size()), mPoints2(pKF2->mvKeysUn.size()),
          mMatch12(pKF1->mvKeysUn.size(), -1), mLevelSigma2(pKF1->mvLevelSigma2), mN1((int)vpMatched12.size()), mbReset(true), mbFailed(false)
    {
        static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
        if (!mKeys1.empty()) std::memcpy(mKeys1.data(), pKF1->mvKeysUn.data(), sizeof(amos_keypoint) * mKeys1.size());
        if (!mKeys2.empty()) std::memcpy(mKeys2.data(), pKF2->mvKeysUn.data(), sizeof(amos_keypoint) * mKeys2.size());
        const amos_sim3_point none = {{0.f, 0.f, 0.f}, AMOS_SIM3_POINT_SKIP};
        std::fill(mPoints1.begin(), mPoints1.end(), none);
        std::fill(mPoints2.begin(), mPoints2.end(), none);
        const std::vector<MapPointT *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        const int n1 = (int)mKeys1.size(), n2 = (int)mKeys2.size();
        for (int i1 = 0; i1 < mN1 && i1 < n1 && i1 < (int)vpKeyFrameMP1.size(); i1++) {  // Sim3Solver.cc:78-127
            MapPointT *pMP2 = vpMatched12[i1];
            if (!pMP2) continue;
            MapPointT *pMP1 = vpKeyFrameMP1[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0 || indexKF1 >= n1 || indexKF2 >= n2) continue;
            mKeys1[i1].octave = pKF1->mvKeysUn[indexKF1].octave;  // kp1 = mvKeysUn[indexKF1]
            Fill(mPoints1[i1], pMP1);
            Fill(mPoints2[indexKF2], pMP2);
            mMatch12[i1] = indexKF2;
        }
        FillCamera(mCameras[0], pKF1);
        FillCamera(mCameras[1], pKF2);
        std::memset(&mParams, 0, sizeof(mParams));
        mParams.fix_scale = bFixScale ? 1 : 0;
        mParams.seed = seed;
        mParams.enabled = 1;
        std::memset(&mResult, 0, sizeof(mResult));
        mState.assign(Sim3StateBytes(n1), 0);
        SetRansacParameters();
    }

    // takes effect with the next iterate(), which starts the solver over (the reference sets its parameters once, before the first iterate)
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mParams.probability = probability; mParams.min_inliers = minInliers; mParams.max_iterations = maxIterations;
        mbReset = true;
    }

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers)
    {
        bool bFlag;
        return iterate(mParams.max_iterations, bFlag, vbInliers12, nInliers);
    }

    // Sim3Solver.cc:199-285.  An empty matrix with bNoMore set and Failed() true: the library refused the call.
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false;
        vbInliers.assign((size_t)mN1, false);
        nInliers = 0;
        const int n1 = (int)mKeys1.size(), n2 = (int)mKeys2.size();
        mParams.n_iterations = nIterations;
        mParams.reset = mbReset ? 1 : 0;
        std::vector<uint8_t> inlier((size_t)n1, 0);
        std::vector<int32_t> matchOut((size_t)n1, -1);
        mbFailed = Sim3Arrays(mKeys1.data(), mPoints1.data(), n1, mKeys2.data(), mPoints2.data(), n2, mCameras, mMatch12.data(), mLevelSigma2.data(),
                              (int)mLevelSigma2.size(), mParams, mState.data(), &mResult, inlier.data(), matchOut.data()) != 0 || mResult.code != 0;
        if (mbFailed) {
            bNoMore = true;
            return cv::Mat();
        }
        mbReset = false;
        bNoMore = mResult.no_more != 0;
        if (!mResult.has_sim3) return cv::Mat();
        nInliers = mResult.n_inliers;
        for (int i = 0; i < n1 && i < mN1; i++) vbInliers[i] = inlier[i] != 0;
        cv::Mat T12 = cv::Mat::zeros(4, 4, CV_32F);
        for (int k = 0; k < 16; k++) T12.at<float>(k / 4, k % 4) = mResult.T12[k];
        return T12;
    }

    // the Sim3 of the last iterate() that returned one (LoopClosing reads them only then); zeros after a call that returned none
    cv::Mat GetEstimatedRotation()
    {
        cv::Mat R = cv::Mat::zeros(3, 3, CV_32F);
        for (int k = 0; k < 9; k++) R.at<float>(k / 3, k % 3) = mResult.R12[k];
        return R;
    }
    cv::Mat GetEstimatedTranslation()
    {
        cv::Mat t = cv::Mat::zeros(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) t.at<float>(k, 0) = mResult.t12[k];
        return t;
    }
    float GetEstimatedScale() { return mResult.s12; }

    bool Failed() const { return mbFailed; }
    const amos_sim3_result &LastResult() const { return mResult; }
    // the arrays the constructor built, for the tests
    const std::vector<amos_keypoint> &Keys1() const { return mKeys1; }
    const std::vector<amos_sim3_point> &Points1() const { return mPoints1; }
    const std::vector<amos_sim3_point> &Points2() const { return mPoints2; }
    const std::vector<int32_t> &Match12() const { return mMatch12; }

private:
    static void Fill(amos_sim3_point &p, MapPointT *pMP)
    {
        const cv::Mat P = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) p.pos[k] = P.template at<float>(k, 0);
        p.flags = 0;
    }
    static void FillCamera(amos_sim3_camera &c, KeyFrameT *pKF)
    {
        const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation();
        for (int k = 0; k < 9; k++) c.Rcw[k] = R.template at<float>(k / 3, k % 3);
        for (int k = 0; k < 3; k++) c.tcw[k] = t.template at<float>(k, 0);
        c.fx = pKF->fx; c.fy = pKF->fy; c.cx = pKF->cx; c.cy = pKF->cy;
    }

    std::vector<amos_keypoint> mKeys1, mKeys2;
    std::vector<amos_sim3_point> mPoints1, mPoints2;
    std::vector<int32_t> mMatch12;
    std::vector<float> mLevelSigma2;
    std::vector<uint8_t> mState;
    amos_sim3_camera mCameras[2];
    amos_sim3_params mParams;
    amos_sim3_result mResult;
    int mN1;
    bool mbReset, mbFailed;
};

}  // namespace ORB_SLAM2

#endif
