// reloc_pnp_capi.cc -- two things behind C entry points:
//   1. the HOST COMPILATION of the relocalisation PnP solver: amos-slam_amd/csrc/amos_pnp_core.h compiled as plain C++ (no HIP), its solver
//      pieces (solver_parameters, solver_draw4, epnp_serial with the direct pixel policy, solver_inlier, solver_tcw) put together as a
//      literal single-threaded PnPsolver (PnPsolver.cc:120-458).  The CPU tests hold it to tests/reloc_pnp_restatement.py bit for bit, so
//      the arithmetic the kernel shares is checked without a GPU; tools/reloc_pnp_bench.py times it.
//   2. ORB_SLAM2::DevicePnPsolver (amos-slam_amd/host/FrameRelocalizationPnP.h) driven on stand-in Frame / MapPoint objects.
// Test harness: links the product library, never the other way round.
#include <chrono>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../amos-slam_amd/csrc/amos_pnp_core.h"
#include "../../include/amos_frontend.h"
#include "../host/ref_standins.h"
#include "../../amos-slam_amd/host/FrameRelocalizationPnP.h"

using namespace ORB_SLAM2;
namespace pnp = amos::pnp;

namespace
{
using namespace amos_standins;
thread_local std::string g_error;

struct HostSolver {
    int nFeatures = 0, N = 0, status = 0, code = 0;
    std::vector<float> X, Y, Z, u, v, maxErr;
    std::vector<int> key;
    double fu = 0, fv = 0, uc = 0, vc = 0;
    uint64_t rng = 0;
    int minInliers = 0, maxIts = 0, iterations = 0, bestInliers = 0;
    float eps = 0;
    std::vector<uint8_t> cur, best, refined;
    float bestTcw[12] = {}, refinedTcw[12] = {};
    int nRefined = 0;
    std::vector<double> scr;
    double MtM[144], E[144];

    int check(const double *Rt, std::vector<uint8_t> &mask) const
    {
        int count = 0;
        for (int i = 0; i < N; i++) {
            mask[i] = pnp::solver_inlier(Rt, X[i], Y[i], Z[i], u[i], v[i], fu, fv, uc, vc, maxErr[i]) ? 1 : 0;
            count += mask[i];
        }
        return count;
    }
    void solve(const int *idx, int m, double *Rt)
    {
        scr.resize((size_t)m * pnp::kEpnpScratch);
        pnp::epnp_serial<pnp::PixelDirect>(m, [&](int j, double *pw, float &pu, float &pv) {
            const int i = idx[j];
            pw[0] = X[i]; pw[1] = Y[i]; pw[2] = Z[i];
            pu = u[i]; pv = v[i];
        }, fu, fv, uc, vc, scr.data(), MtM, E, Rt);
    }
    bool refine()  // PnPsolver.cc:366-418
    {
        std::vector<int> idx;
        for (int i = 0; i < N; i++)
            if (best[i]) idx.push_back(i);
        double Rt[12];
        solve(idx.data(), (int)idx.size(), Rt);
        nRefined = check(Rt, refined);
        pnp::solver_tcw(Rt, refinedTcw);
        return nRefined > minInliers;
    }
};

void fill_result(const HostSolver &s, amos_reloc_pnp_result *r, uint8_t *inlier, const float *Tcw, const std::vector<uint8_t> *mask, int n, bool refined,
                 bool noMore, int cur)
{
    std::memset(r, 0, sizeof(*r));
    if (s.nFeatures) std::memset(inlier, 0, (size_t)s.nFeatures);
    r->n_correspondences = s.N; r->min_inliers = s.minInliers; r->max_iterations = s.maxIts;
    r->iterations = s.iterations; r->iterations_call = cur; r->best_inliers = s.bestInliers; r->status = s.status;
    r->no_more = noMore ? 1 : 0;
    if (Tcw) {
        r->has_pose = 1; r->refined = refined ? 1 : 0; r->n_inliers = n;
        for (int k = 0; k < 12; k++) r->Tcw[k] = Tcw[k];
        for (int i = 0; i < s.N; i++)
            if ((*mask)[i]) inlier[s.key[i]] = 1;
    }
}
}  // namespace

extern "C" {

const char *amos_host_reloc_pnp_last_error(void) { return g_error.c_str(); }

// the constructor and SetRansacParameters(params) of the host-compiled solver; NULL: out of memory
void *amos_host_pnp_solver_create(const amos_keypoint *kps, int n, const int32_t *bow_match, const amos_reloc_point *points, int n_points,
                                  const float *level_sigma2, int n_levels, const amos_reloc_pnp_params *par)
{
    try {
        HostSolver *s = new HostSolver();
        s->nFeatures = n;
        std::vector<float> sigma2;
        int total = 0;
        for (int i = 0; i < n; i++) {
            const int j = bow_match[i];
            if (j < 0) continue;
            if (j >= n_points) { s->status |= 2; continue; }
            if (points[j].flags & AMOS_RELOC_POINT_SKIP) continue;
            const int oct = kps[i].octave;
            if (oct < 0 || oct >= n_levels) { s->status |= 1; continue; }
            total++;
            if (total > pnp::kSolverMaxPoints) continue;
            s->key.push_back(i);
            s->X.push_back(points[j].pos[0]); s->Y.push_back(points[j].pos[1]); s->Z.push_back(points[j].pos[2]);
            s->u.push_back(kps[i].x); s->v.push_back(kps[i].y);
            sigma2.push_back(level_sigma2[oct]);
        }
        s->N = total;
        if (total > pnp::kSolverMaxPoints) { s->code = -3; return s; }
        s->fu = (double)par->fx; s->fv = (double)par->fy; s->uc = (double)par->cx; s->vc = (double)par->cy;
        s->rng = par->seed;
        pnp::solver_parameters(s->N, par->probability, par->min_inliers, par->max_iterations, par->epsilon, s->minInliers, s->maxIts, s->eps);
        s->maxErr.resize(s->N);
        for (int i = 0; i < s->N; i++) s->maxErr[i] = pnp::fmul(sigma2[i], par->th2);
        s->cur.assign(s->N, 0); s->best.assign(s->N, 0); s->refined.assign(s->N, 0);
        return s;
    } catch (const std::exception &e) {
        g_error = e.what();
        return nullptr;
    }
}

void amos_host_pnp_solver_destroy(void *h) { delete static_cast<HostSolver *>(h); }

// PnPsolver::iterate(n_iterations), literally and on one thread; inlier [n features]; rng_state: the generator behind the call
int amos_host_pnp_solver_iterate(void *h, int n_iterations, amos_reloc_pnp_result *result, uint8_t *inlier, uint64_t *rng_state)
{
    try {
        HostSolver &s = *static_cast<HostSolver *>(h);
        if (s.code) {
            std::memset(result, 0, sizeof(*result));
            result->code = s.code; result->n_correspondences = s.N; result->status = s.status;
            if (rng_state) *rng_state = s.rng;
            return 0;
        }
        int cur = 0;
        bool done = false;
        if (s.N < s.minInliers) {
            fill_result(s, result, inlier, nullptr, nullptr, 0, false, true, 0);
            done = true;
        }
        while (!done && (s.iterations < s.maxIts || cur < n_iterations)) {
            cur++;
            s.iterations++;
            int idx[4];
            pnp::solver_draw4(s.rng, s.N, idx);
            double Rt[12];
            s.solve(idx, 4, Rt);
            const int count = s.check(Rt, s.cur);
            if (count >= s.minInliers) {
                if (count > s.bestInliers) {
                    s.best = s.cur;
                    s.bestInliers = count;
                    pnp::solver_tcw(Rt, s.bestTcw);
                }
                if (s.refine()) {
                    fill_result(s, result, inlier, s.refinedTcw, &s.refined, s.nRefined, true, false, cur);
                    done = true;
                }
            }
        }
        if (!done) {
            const bool noMore = s.iterations >= s.maxIts;
            if (noMore && s.bestInliers >= s.minInliers) fill_result(s, result, inlier, s.bestTcw, &s.best, s.bestInliers, false, true, cur);
            else fill_result(s, result, inlier, nullptr, nullptr, 0, false, noMore, cur);
        }
        if (rng_state) *rng_state = s.rng;
        return 0;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

// the pieces on their own, for the CPU tests
void amos_host_pnp_draw4(uint64_t *rng, int N, int32_t *idx)
{
    int out[4];
    pnp::solver_draw4(*rng, N, out);
    for (int k = 0; k < 4; k++) idx[k] = out[k];
}

void amos_host_pnp_parameters(int N, double probability, int min_inliers, int max_iterations, float epsilon, int32_t *out_min, int32_t *out_its, float *out_eps)
{
    int a, b;
    pnp::solver_parameters(N, probability, min_inliers, max_iterations, epsilon, a, b, *out_eps);
    *out_min = a; *out_its = b;
}

// ORB_SLAM2::DevicePnPsolver<Frame, MapPoint> on stand-ins: a frame of n features (keys_un, camera, level_sigma2), vp_matches [n] = index
// into the point table (world [n_points][3], bad [n_points]) or -1.  SetRansacParameters(probability, min_inliers, max_iterations, 4,
// epsilon, th2), then n_calls times iterate(n_iterations).  Out per call: Tcw [16] (zeros when empty), has_pose, no_more, n_inliers,
// inliers [n] (vbInliers; all zero when it came back empty).  ms: mean wall time of one iterate.  Returns 0.
int amos_host_pnp_dropin(const amos_keypoint *keys_un, int n, float fx, float fy, float cx, float cy, const float *level_sigma2, int n_levels,
                         const float *world, const uint8_t *bad, int n_points, const int32_t *vp_matches, uint64_t seed, double probability,
                         int min_inliers, int max_iterations, float epsilon, float th2, int n_iterations, int n_calls, float *Tcw, int32_t *has_pose,
                         int32_t *no_more, int32_t *n_inliers, uint8_t *inliers, double *ms)
{
    try {
        std::vector<MapPoint> pts((size_t)n_points);
        for (int i = 0; i < n_points; i++) {
            for (int k = 0; k < 3; k++) pts[i].mWorldPos.at<float>(k, 0) = world[3 * i + k];
            pts[i].mbBad = bad && bad[i];
        }
        Frame F;
        F.N = n;
        F.mvKeysUn.resize(n);
        if (n) std::memcpy(F.mvKeysUn.data(), keys_un, sizeof(amos_keypoint) * (size_t)n);
        F.fx = fx; F.fy = fy; F.cx = cx; F.cy = cy;
        F.mnScaleLevels = n_levels;
        F.mvLevelSigma2.assign(level_sigma2, level_sigma2 + n_levels);
        std::vector<MapPoint *> vpMatches((size_t)n, static_cast<MapPoint *>(NULL));
        for (int i = 0; i < n; i++)
            if (vp_matches[i] >= 0) vpMatches[i] = &pts[vp_matches[i]];
        DevicePnPsolver<Frame, MapPoint> solver(F, vpMatches, seed);
        solver.SetRansacParameters(probability, min_inliers, max_iterations, 4, epsilon, th2);
        double total = 0;
        for (int call = 0; call < n_calls; call++) {
            bool bNoMore = false;
            std::vector<bool> vbInliers;
            int nInliers = 0;
            const auto t0 = std::chrono::steady_clock::now();
            cv::Mat T = solver.iterate(n_iterations, bNoMore, vbInliers, nInliers);
            total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (solver.Failed()) { g_error = amos_last_error(); return -101; }
            has_pose[call] = T.empty() ? 0 : 1;
            no_more[call] = bNoMore ? 1 : 0;
            n_inliers[call] = nInliers;
            for (int k = 0; k < 16; k++) Tcw[16 * call + k] = T.empty() ? 0.f : T.at<float>(k / 4, k % 4);
            for (int i = 0; i < n; i++) inliers[(size_t)call * n + i] = (i < (int)vbInliers.size() && vbInliers[i]) ? 1 : 0;
        }
        if (ms) *ms = n_calls > 0 ? total / n_calls : 0.0;
        return 0;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

}  // extern "C"
