// new_points_capi.cc -- C entry points for the new-map-point tests: the host compilation of amos-slam_amd/csrc/amos_new_points_core.h (its
// functions one by one, and new_points_host.h's complete loop over pairs and matches), and ORB_SLAM2::CreateNewMapPointCandidates
// (amos-slam_amd/host/KeyFrameNewPoints.h) on stand-in KeyFrame objects beside what the mapping thread ran before it: the drop-in search
// for all neighbours followed by the host-compiled core looped over neighbours and matches.  Test harness: links the product library,
// never the other way round.  The keyframe struct is that of tests/host/host_capi.cc (host_binding.TestKF).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/amos_host_types.h"
#include "../../amos-slam_amd/host/ORBmatcher.h"
#include "../../amos-slam_amd/host/ORBmatcher_adaptors.h"
#include "../host/ref_standins.h"
#include "../../amos-slam_amd/host/KeyFrameSearch.h"
#include "../../amos-slam_amd/host/KeyFrameNewPoints.h"
#include "new_points_host.h"

using namespace ORB_SLAM2;

extern "C" {
struct amos_test_camera {
    float fx, fy, cx, cy, mb, mbf;
    float min_x, max_x, min_y, max_y;
    float Tcw[16];
    int32_t n_levels;
    float scale_factors[AMOS_MAX_LEVELS];
};
struct amos_test_kf {
    amos_test_camera cam;
    int32_t n;
    const amos_keypoint *keys, *keys_un;
    const uint8_t *desc;
    const float *u_right;     // NULL: monocular (mvuRight all -1)
    const int32_t *point_of;  // n: >= 0: the feature has a map point
    int32_t n_nodes;
    const uint32_t *node_ids;
    const int32_t *node_off, *node_idx;
};
}

namespace
{
// the stand-in keyframe with the members CreateNewMapPoints reads beside the searches'
class KeyFrame : public amos_standins::KeyFrame
{
public:
    std::vector<float> mvDepth;
    float invfx = 0, invfy = 0, mfScaleFactor = 0;
};

thread_local std::string g_error;
amos_standins::MapPoint g_point;  // what a feature with a map point points to

void fill_keyframe(KeyFrame &kf, const amos_test_kf *k, const float *depth)
{
    const int n = k->n;
    kf.N = n;
    kf.mvKeys.resize(n);
    kf.mvKeysUn.resize(n);
    if (n) {
        std::memcpy(kf.mvKeys.data(), k->keys, sizeof(amos_keypoint) * n);
        std::memcpy(kf.mvKeysUn.data(), k->keys_un, sizeof(amos_keypoint) * n);
    }
    kf.mDescriptors = cv::Mat(std::max(n, 1), 32, CV_8U);
    if (n) std::memcpy(kf.mDescriptors.data, k->desc, (size_t)32 * n);
    if (k->u_right) kf.mvuRight.assign(k->u_right, k->u_right + n);
    else kf.mvuRight.assign(n, -1.f);
    if (depth) kf.mvDepth.assign(depth, depth + n);
    const amos_test_camera &c = k->cam;
    kf.fx = c.fx; kf.fy = c.fy; kf.cx = c.cx; kf.cy = c.cy; kf.mb = c.mb; kf.mbf = c.mbf;
    kf.invfx = 1.0f / c.fx; kf.invfy = 1.0f / c.fy;  // Frame.cc
    kf.mnScaleLevels = c.n_levels;
    kf.mfScaleFactor = c.scale_factors[1];
    kf.mvScaleFactors.assign(c.scale_factors, c.scale_factors + c.n_levels);
    kf.mvLevelSigma2.resize(c.n_levels);
    for (int l = 0; l < c.n_levels; l++) kf.mvLevelSigma2[l] = c.scale_factors[l] * c.scale_factors[l];  // ORBextractor.cc:522-533
    for (int j = 0; j < k->n_nodes; j++) {
        std::vector<unsigned int> &v = kf.mFeatVec[k->node_ids[j]];
        for (int e = k->node_off[j]; e < k->node_off[j + 1]; e++) v.push_back((unsigned int)k->node_idx[e]);
    }
    kf.mvpMapPoints.assign(n, static_cast<amos_standins::MapPoint *>(NULL));
    for (int i = 0; i < n; i++)
        if (k->point_of && k->point_of[i] >= 0) kf.mvpMapPoints[i] = &g_point;
    kf.Tcw = cv::Mat(4, 4, CV_32F);
    std::memcpy(kf.Tcw.data, c.Tcw, sizeof(float) * 16);
    const amos_adapt::V3 ow = amos_adapt::centre(amos_adapt::pose_of(kf.Tcw));  // KeyFrame::SetPose
    kf.Ow = cv::Mat(3, 1, CV_32F);
    kf.Ow.at<float>(0, 0) = ow.x; kf.Ow.at<float>(1, 0) = ow.y; kf.Ow.at<float>(2, 0) = ow.z;
}

// what the mapping thread ran before: one search call for the neighbours that pass the gate, then LocalMapping.cc:410-597 per neighbour
// and match on the host; a keyframe-1 feature that produced a point is not given a second one
int parent_new_points(KeyFrame *pKF1, const std::vector<KeyFrame *> &neigh, std::vector<std::vector<NewMapPointCandidate> > &vvNew, bool checkOri)
{
    using namespace amos_adapt;
    const int n2 = (int)neigh.size();
    vvNew.assign(n2, std::vector<NewMapPointCandidate>());
    const amos_kf_camera c1 = kf_camera_of(pKF1);
    std::vector<amos_kf_camera> c2(n2);
    std::vector<int> kept;
    std::vector<KeyFrame *> keptKFs;
    std::vector<cv::Mat> F;
    for (int k = 0; k < n2; k++) {
        c2[k] = kf_camera_of(neigh[k]);
        amos_kf_geometry g;
        if (!amos::newpt::pair_geometry(c1, c2[k], &g)) continue;
        kept.push_back(k);
        keptKFs.push_back(neigh[k]);
        cv::Mat f(3, 3, CV_32F);
        std::memcpy(f.data, g.f12, sizeof(float) * 9);
        F.push_back(f);
    }
    if (kept.empty()) return 0;
    std::vector<std::vector<std::pair<size_t, size_t> > > pairs;
    if (SearchForTriangulation(pKF1, keptKFs, F, pairs, false, checkOri) < 0) return -1;
    std::vector<uint8_t> made(pKF1->N, 0);
    int total = 0;
    for (size_t e = 0; e < kept.size(); e++) {
        KeyFrame *pKF2 = keptKFs[e];
        for (size_t m = 0; m < pairs[e].size(); m++) {
            const size_t i1 = pairs[e][m].first, i2 = pairs[e][m].second;
            amos::newpt::Feature f1, f2;
            KeyFrame *kfs[2] = {pKF1, pKF2};
            const size_t idx[2] = {i1, i2};
            amos::newpt::Feature *fs[2] = {&f1, &f2};
            for (int s = 0; s < 2; s++) {
                fs[s]->x = kfs[s]->mvKeysUn[idx[s]].pt.x; fs[s]->y = kfs[s]->mvKeysUn[idx[s]].pt.y; fs[s]->octave = kfs[s]->mvKeysUn[idx[s]].octave;
                fs[s]->rawX = kfs[s]->mvKeys[idx[s]].pt.x; fs[s]->rawY = kfs[s]->mvKeys[idx[s]].pt.y;
                fs[s]->uRight = kfs[s]->mvuRight[idx[s]];
                fs[s]->depth = fs[s]->uRight >= 0 ? kfs[s]->mvDepth[idx[s]] : -1.0f;
            }
            NewMapPointCandidate c;
            const int v = amos::newpt::triangulate_match(c1, c2[kept[e]], f1, f2, pKF1->mvScaleFactors.data(), pKF1->mvLevelSigma2.data(),
                                                         (int)pKF1->mvScaleFactors.size(), c.x3D);
            if (v > AMOS_NEW_POINT_UNPROJECTED_2 || made[i1]) continue;
            made[i1] = 1;
            c.idx1 = i1; c.idx2 = i2; c.source = v;
            vvNew[kept[e]].push_back(c);
            total++;
        }
    }
    return total;
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

extern "C" {

const char *amos_host_new_points_last_error(void) { return g_error.c_str(); }

// ---- the core header's functions
int amos_host_new_points_geometry(const amos_kf_camera *c1, const amos_kf_camera *c2, amos_kf_geometry *g) { return amos::newpt::pair_geometry(*c1, *c2, g) ? 1 : 0; }
float amos_host_new_points_cos_stereo(float mb, float d) { return amos::newpt::cos_stereo_parallax(mb, d); }
// which = 0: jacobi_sym4; 1: pnp::jacobi_sym(., ., 4).  S [16] is replaced by what the sweeps leave, V [16] receives the eigenvectors
void amos_host_new_points_jacobi(double *S, double *V, int which)
{
    if (which == 0) {
        double s[16], v[16];
        std::memcpy(s, S, sizeof(s));
        amos::newpt::jacobi_sym4(s, v);
        std::memcpy(S, s, sizeof(s));
        std::memcpy(V, v, sizeof(v));
    } else
        amos::pnp::jacobi_sym(S, V, 4);
}
void amos_host_new_points_null_vector(const float *A, float *v) { amos::newpt::null_vector4(A, v); }
int amos_host_new_points_dehomogenise(const float *v, float *x3D) { return amos::newpt::dehomogenise(v, x3D) ? 1 : 0; }
int amos_host_new_points_scale_gate(const amos_kf_camera *c1, const amos_kf_camera *c2, int o1, int o2, const float *scale, const float *X)
{
    return amos::newpt::scale_gate(*c1, *c2, o1, o2, scale, X);
}

// ---- the complete host loop on the arrays of amos_match_new_points_batch_device
void amos_host_new_points_core(const new_points_host::Input *in, amos_new_point *out_new, int32_t *out_verdict, amos_new_points_stats *out_stats)
{
    new_points_host::run(*in, out_new, out_verdict, out_stats);
}

// ---- CreateNewMapPointCandidates on stand-in keyframes.  which = 0: the drop-in; 1: the parent (drop-in search + the host-compiled core).
// depths[k]: mvDepth of keyframe k (k = 0: keyframe 1) or NULL.  out [n2][cap] records, counts [n2]; ms[rep] = the wall time of run rep.
// Returns the call's return value (-1: the library refused; the text is in amos_host_new_points_last_error).
int amos_host_new_points_dropin(const amos_test_kf *kf1, const amos_test_kf *const *kf2s, int n2, const float *const *depths, int check_orientation,
                                int which, int repeat, amos_new_point *out, int32_t *counts, amos_new_points_stats *stats, int cap, double *ms)
{
    try {
        KeyFrame K1;
        fill_keyframe(K1, kf1, depths[0]);
        std::vector<KeyFrame> K2(n2);
        std::vector<KeyFrame *> p2(n2);
        for (int k = 0; k < n2; k++) {
            fill_keyframe(K2[k], kf2s[k], depths[k + 1]);
            p2[k] = &K2[k];
        }
        std::vector<std::vector<NewMapPointCandidate> > vv;
        std::vector<amos_new_points_stats> st;
        int ret = 0;
        for (int rep = 0; rep < std::max(repeat, 1); rep++) {
            const double t0 = now_ms();
            ret = which == 0 ? CreateNewMapPointCandidates(&K1, p2, vv, check_orientation != 0, &st) : parent_new_points(&K1, p2, vv, check_orientation != 0);
            if (ms) ms[rep] = now_ms() - t0;
            if (ret < 0) { g_error = amos_last_error(); return -1; }
        }
        for (int k = 0; k < n2; k++) {
            if ((int)vv[k].size() > cap) { g_error = "more candidates than the output holds"; return -3; }
            counts[k] = (int32_t)vv[k].size();
            for (size_t e = 0; e < vv[k].size(); e++) {
                amos_new_point &r = out[(size_t)k * cap + e];
                r.idx1 = (int32_t)vv[k][e].idx1; r.idx2 = (int32_t)vv[k][e].idx2;
                r.x = vv[k][e].x3D[0]; r.y = vv[k][e].x3D[1]; r.z = vv[k][e].x3D[2];
                r.verdict = vv[k][e].source;
            }
            if (stats && which == 0) stats[k] = st[k];
        }
        return ret;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

}  // extern "C"
