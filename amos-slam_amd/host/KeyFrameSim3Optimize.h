// KeyFrameSim3Optimize.h -- Optimizer::OptimizeSim3 (Optimizer.cc:1364-1590) on the device: both optimisations and both inlier checks as ONE
// call of the C ABI (amos_match_sim3_optimize of include/amos_frontend.h: one upload, one launch, one download).  The host keeps the pointer
// work: the map-point rows of the two keyframes, GetIndexInKeyFrame for the entries of vpMatches1, and the write-back of the cleared
// entries and of the Sim3.  The template gathers the arrays from the caller's KeyFrame / MapPoint objects.
#ifndef KEYFRAMESIM3OPTIMIZE_H
#define KEYFRAMESIM3OPTIMIZE_H

#include <cstring>
#include <vector>

#include "../../include/amos_frontend.h"
#include "KeyFrameSim3Search.h"  // amos_sim3_search::camera_of
#include "amos_cv.h"

namespace ORB_SLAM2
{

// The call itself on the calling thread's pooled matcher handle (FrameLocalPoints.h).  0, or -1 with the text in amos_last_error().
int OptimizeSim3Arrays(const amos_keypoint *kps1, const amos_sim3_point *points1, int n1, const amos_keypoint *kps2, const amos_sim3_point *points2,
                       int n2, const amos_sim3_camera *cameras, const int32_t *match12, const float *invLevelSigma2, int nLevels,
                       const amos_sim3_opt_pair &pair, int32_t *matchOut, amos_sim3_opt_result *result);

// How the drop-in reads and writes the caller's Sim3: rotation as x, y, z, w, then translation, then scale.  The default uses the element
// access of g2o::Sim3 (sim3.h:239-264: [0 .. 3] r.coeffs(), [4 .. 6] t, [7] s); specialise it for another type.
template <class Sim3T>
struct Sim3Access {
    static void Read(const Sim3T &S, double *q, double *t, double *s)
    {
        for (int i = 0; i < 4; i++) q[i] = S[i];
        for (int i = 0; i < 3; i++) t[i] = S[4 + i];
        *s = S[7];
    }
    static void Write(Sim3T &S, const double *q, const double *t, double s)
    {
        for (int i = 0; i < 4; i++) S[i] = q[i];
        for (int i = 0; i < 3; i++) S[4 + i] = t[i];
        S[7] = s;
    }
};

namespace amos_sim3_optimize
{
template <class MapPointT>
inline amos_sim3_point point_of(MapPointT *pMP)
{
    amos_sim3_point p;
    std::memset(&p, 0, sizeof(p));
    if (!pMP || pMP->isBad()) {
        p.flags = AMOS_SIM3_POINT_SKIP;
        return p;
    }
    const cv::Mat P = pMP->GetWorldPos();
    for (int k = 0; k < 3; k++) p.pos[k] = P.template at<float>(k, 0);
    return p;
}

// Quaterniond::toRotationMatrix, rounded once to float: the R12 the device takes
inline void rotation_of(const double *q, float *R)
{
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = (float)(1.0 - (tyy + tzz)); R[1] = (float)(txy - twz); R[2] = (float)(txz + twy);
    R[3] = (float)(txy + twz); R[4] = (float)(1.0 - (txx + tzz)); R[5] = (float)(tyz - twx);
    R[6] = (float)(txz - twy); R[7] = (float)(tyz + twx); R[8] = (float)(1.0 - (txx + tyy));
}
}  // namespace amos_sim3_optimize

// The reference's argument list and return value (LoopClosing.cc:461).  Returns nIn, or -1 when the library refused; then vpMatches1 and
// g2oS12 are as they were.  g2oS12 is written when both optimisations ran; a return of 0 ahead of the second leaves it, as the reference does.
template <class KeyFrameT, class MapPointT, class Sim3T>
int OptimizeSim3(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches1, Sim3T &g2oS12, const float th2, const bool bFixScale)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(amos_keypoint), "cv::KeyPoint and amos_keypoint share one layout");
    const std::vector<MapPointT *> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    const int N1 = (int)vpMapPoints1.size(), N2 = (int)vpMapPoints2.size();
    std::vector<amos_sim3_point> points1(N1 > 0 ? N1 : 1), points2(N2 > 0 ? N2 : 1);
    for (int i = 0; i < N1; i++) points1[i] = amos_sim3_optimize::point_of(vpMapPoints1[i]);
    for (int j = 0; j < N2; j++) points2[j] = amos_sim3_optimize::point_of(vpMapPoints2[j]);
    std::vector<int32_t> row(N1 > 0 ? N1 : 1, -1), out(N1 > 0 ? N1 : 1, -1);
    const int nMatches = (int)vpMatches1.size() < N1 ? (int)vpMatches1.size() : N1;
    for (int i = 0; i < nMatches; i++) {  // :1429-1447
        MapPointT *pMP2 = vpMatches1[i];
        if (!pMP2) continue;
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (i2 < 0 || i2 >= N2) { row[i] = AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE; continue; }
        row[i] = i2;
        points2[i2] = amos_sim3_optimize::point_of(pMP2);  // the reference reads pMP2 itself (KF2's point at feature i2, normally)
    }
    const amos_sim3_camera cams[2] = {amos_sim3_search::camera_of(pKF1), amos_sim3_search::camera_of(pKF2)};
    double q[4], t[3], s;
    Sim3Access<Sim3T>::Read(g2oS12, q, t, &s);
    amos_sim3_opt_pair pair;
    amos_sim3_optimize::rotation_of(q, pair.R12);
    for (int k = 0; k < 3; k++) pair.t12[k] = (float)t[k];
    pair.s12 = (float)s; pair.th2 = th2; pair.fix_scale = bFixScale ? 1 : 0; pair.enabled = 1;
    amos_sim3_opt_result res;
    if (OptimizeSim3Arrays(reinterpret_cast<const amos_keypoint *>(pKF1->mvKeysUn.data()), points1.data(), N1,
                           reinterpret_cast<const amos_keypoint *>(pKF2->mvKeysUn.data()), points2.data(), N2, cams, row.data(),
                           pKF1->mvInvLevelSigma2.data(), (int)pKF1->mvInvLevelSigma2.size(), pair, out.data(), &res) != 0 || res.code != 0)
        return -1;
    for (int i = 0; i < nMatches; i++)  // :1538-1547, :1575-1579
        if (row[i] >= 0 && out[i] == -1) vpMatches1[i] = static_cast<MapPointT *>(NULL);
    if (res.rounds == 2) Sim3Access<Sim3T>::Write(g2oS12, res.q, res.t, res.s);
    return res.n_inliers;
}

}  // namespace ORB_SLAM2

#endif
