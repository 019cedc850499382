// sim3_host_solver.h -- the HOST COMPILATION of the loop-closing Sim3 solver: amos-slam_amd/csrc/amos_sim3_core.h compiled as plain C++
// (no HIP), its pieces (sim3_parameters, sim3_draw3, sim3_horn, sim3_inlier) put together as a literal single-threaded Sim3Solver
// (Sim3Solver.cc:48-285).  Shared by sim3_capi.cc (the test library) and sim3_core_main.cc (the stand-alone program).
#pragma once

#include <cstring>
#include <vector>

#include "../../amos-slam_amd/csrc/amos_sim3_core.h"
#include "../../include/amos_frontend.h"

namespace sim3_host
{
namespace sim3 = amos::sim3;

struct Solver {
    int nFeatures = 0, N = 0, status = 0, code = 0;
    std::vector<sim3::Correspondence> corr;
    std::vector<int> key;
    std::vector<int32_t> match12;
    float K1[4] = {}, K2[4] = {};
    uint64_t rng = 0;
    int minInliers = 0, maxIts = 0, iterations = 0, bestInliers = 0;
    bool fixScale = false;
    std::vector<uint8_t> cur, best;
    sim3::Hypothesis bestH = {};

    // the constructor (Sim3Solver.cc:48-140) and SetRansacParameters (:143-196)
    Solver(const amos_keypoint *kps1, const amos_sim3_point *points1, int n1, const amos_keypoint *kps2, const amos_sim3_point *points2, int n2,
           const amos_sim3_camera *cameras, const int32_t *m12, const float *levelSigma2, int nLevels, const amos_sim3_params &par)
    {
        nFeatures = n1;
        match12.assign(m12, m12 + n1);
        const amos_sim3_camera &c1 = cameras[0], &c2 = cameras[1];
        const float k1[4] = {c1.fx, c1.fy, c1.cx, c1.cy}, k2[4] = {c2.fx, c2.fy, c2.cx, c2.cy};
        std::memcpy(K1, k1, sizeof(K1));
        std::memcpy(K2, k2, sizeof(K2));
        int total = 0;
        for (int i = 0; i < n1; i++) {
            const int j = m12[i];
            if (j < 0) continue;
            if (j >= n2) { status |= 2; continue; }
            if ((points1[i].flags & AMOS_SIM3_POINT_SKIP) || (points2[j].flags & AMOS_SIM3_POINT_SKIP)) continue;
            const int o1 = kps1[i].octave, o2 = kps2[j].octave;
            if (o1 < 0 || o1 >= nLevels || o2 < 0 || o2 >= nLevels) { status |= 1; continue; }
            total++;
            if (total > sim3::kMaxCorrespondences) continue;
            sim3::Correspondence c;
            sim3::to_camera(c1.Rcw, c1.tcw, points1[i].pos, c.X1);
            sim3::to_camera(c2.Rcw, c2.tcw, points2[j].pos, c.X2);
            sim3::to_image(c.X1[0], c.X1[1], c.X1[2], K1[0], K1[1], K1[2], K1[3], c.p1[0], c.p1[1]);
            sim3::to_image(c.X2[0], c.X2[1], c.X2[2], K2[0], K2[1], K2[2], K2[3], c.p2[0], c.p2[1]);
            c.maxErr1 = sim3::max_error(levelSigma2[o1]);
            c.maxErr2 = sim3::max_error(levelSigma2[o2]);
            corr.push_back(c);
            key.push_back(i);
        }
        N = total;
        if (total > sim3::kMaxCorrespondences) { code = -3; return; }
        rng = par.seed;
        minInliers = par.min_inliers;
        fixScale = par.fix_scale != 0;
        maxIts = sim3::sim3_parameters(N, par.probability, par.min_inliers, par.max_iterations);
        cur.assign(N, 0);
        best.assign(N, 0);
    }

    void fill(amos_sim3_result *r, uint8_t *inlier, int32_t *matchOut, bool found, bool noMore, int nCur) const
    {
        std::memset(r, 0, sizeof(*r));
        if (nFeatures) std::memset(inlier, 0, (size_t)nFeatures);
        r->n_correspondences = N; r->max_iterations = maxIts; r->iterations = iterations; r->iterations_call = nCur;
        r->best_inliers = bestInliers; r->status = status; r->no_more = noMore ? 1 : 0;
        if (!found) return;
        r->has_sim3 = 1; r->n_inliers = bestInliers;
        for (int k = 0; k < 9; k++) r->R12[k] = bestH.R[k];
        for (int k = 0; k < 3; k++) r->t12[k] = bestH.t[k];
        r->s12 = bestH.s;
        sim3::sim3_T12(bestH, r->T12);
        for (int i = 0; i < N; i++)
            if (best[i]) inlier[key[i]] = 1;
        if (matchOut)
            for (int i = 0; i < nFeatures; i++) matchOut[i] = inlier[i] ? match12[i] : -1;  // LoopClosing.cc:440-447
    }

    // Sim3Solver::iterate(nIterations), literally and on one thread; inlier / matchOut [n1] (matchOut is written only with a Sim3)
    void iterate(int nIterations, amos_sim3_result *r, uint8_t *inlier, int32_t *matchOut)
    {
        if (code) {
            std::memset(r, 0, sizeof(*r));
            r->code = code; r->n_correspondences = N; r->status = status;
            return;
        }
        if (N < minInliers) { fill(r, inlier, matchOut, false, true, 0); return; }
        int nCur = 0;
        while (iterations < maxIts && nCur < nIterations) {
            nCur++;
            iterations++;
            int idx[3];
            sim3::sim3_draw3(rng, N, idx);
            float P1[3][3], P2[3][3];
            for (int c = 0; c < 3; c++)
                for (int k = 0; k < 3; k++) { P1[k][c] = corr[idx[c]].X1[k]; P2[k][c] = corr[idx[c]].X2[k]; }
            sim3::Hypothesis h;
            sim3::sim3_horn(P1, P2, fixScale, h);
            int count = 0;
            for (int i = 0; i < N; i++) {
                cur[i] = sim3::sim3_inlier(h, corr[i], K1, K2) ? 1 : 0;
                count += cur[i];
            }
            if (count >= bestInliers) {
                best = cur;
                bestInliers = count;
                bestH = h;
                if (count > minInliers) { fill(r, inlier, matchOut, true, false, nCur); return; }
            }
        }
        fill(r, inlier, matchOut, false, iterations >= maxIts, nCur);
    }
};

}  // namespace sim3_host
