// amos_ransac.h -- the parts of one RANSAC round that k_fmat_ransac (amos_fmat.hip) and k_pnp_ransac (amos_pnp.hip) share: OpenCV 4.5's
// RANSACPointSetRegistrator::run restated for ONE WORK-GROUP PER PROBLEM working in rounds of drawn-ahead iterations (DESIGN.md
// sections 2 and 4).  A kernel keeps its own sampler test, minimal solver and point layout and reads top to bottom as
//   early exits -> begin -> for (;;) { draw_distinct per slot; solve, one lane per slot; score_models; replay_round; stop? } -> result.
// Device-only, force-inlined; kThreads is the work-group size, kDoubles the doubles of a model (9 or 12), kPerSlot the models one
// subset can give (3 or 1), kModelPoints the subset size (7 or 4), kStatus the ints of a status row (result, inliers, iterations,
// points, then zeros).
#pragma once
#include "amos_block.h"
#include "amos_fmat_core.h"

namespace amos {
namespace ransac {

struct State {   // in LDS, written by one lane between barriers
    int drawn;   // subsets the sampler drew for this round
    int stop;    // after the draw: 0, 1 no subset found (getSubset failed), 2 redraw cap; after the replay: 3 finished, 0 go on
    int result;  // -2 once the redraw cap was hit
    int iter, niters, maxGood;
};

__device__ __forceinline__ void begin(State &s, int maxIters)
{
    if (threadIdx.x == 0) { s.stop = 0; s.result = 0; s.iter = 0; s.niters = maxIters; s.maxGood = 0; }
}

// 1 a model, 0 none, -2 the sampler's cap
__device__ __forceinline__ int result_of(const State &s) { return s.result == -2 ? -2 : (s.maxGood > 0 ? 1 : 0); }

// an exit without a model: zero model, status (result, 0, iterations, n, 0 ..), the cnt mask bytes cleared where there is a mask
template <int kThreads, int kDoubles, int kStatus>
__device__ __forceinline__ void no_model(double *model, int *st, int result, int iterations, int n, uint8_t *mask, int cnt)
{
    const int t = threadIdx.x;
    if (t < kDoubles) model[t] = 0.0;
    if (t == 0) {
        st[0] = result; st[1] = 0; st[2] = iterations; st[3] = n;
        for (int k = 4; k < kStatus; k++) st[k] = 0;
    }
    if (mask) for (int i = t; i < cnt; i += kThreads) mask[i] = 0;
}

// getSubset's draw: K distinct indices of [0, n) from cv::RNG, a duplicate redrawn in place; false once one slot took fm::kRedrawCap
// draws.  Every calling lane advances its own rng.  The draw fills a local array and idx is written once at the end: with idx written
// slot by slot k_fmat_ransac takes three VGPRs more than with the loop written out in the kernel.
template <int K>
__device__ __forceinline__ bool draw_distinct(uint64_t &rng, int n, int *idx)
{
    bool cap = false;
    int v[K] = {};
#pragma unroll
    for (int i = 0; i < K; i++) {
        for (uint32_t draws = 1;; draws++) {
            v[i] = (int)(fm::rng_next(rng) % (uint32_t)n);
            bool dup = false;
#pragma unroll
            for (int j = 0; j < i; j++) dup |= v[i] == v[j];
            if (!dup) break;
            if (draws >= fm::kRedrawCap) { cap = true; break; }
        }
        if (cap) break;
    }
#pragma unroll
    for (int i = 0; i < K; i++) idx[i] = v[i];
    return !cap;
}

// findInliers' count of every model of the round: model m on wave m % waves (live(m) wave-uniform), the n points over the lanes,
// err_of(model in registers, point index) <= thresh2, shuffle-reduced into sCount[m]
template <int kThreads, int kDoubles, typename Live, typename Err>
__device__ __forceinline__ void score_models(const double (*sModel)[kDoubles], int nModels, int n, float thresh2, int *sCount, Live live, Err err_of)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int m = wv; m < nModels; m += kThreads / 64) {
        if (!live(m)) continue;
        double M[kDoubles];
#pragma unroll
        for (int k = 0; k < kDoubles; k++) M[k] = sModel[m][k];
        int count = 0;
        for (int i = lane; i < n; i += 64) count += err_of(M, i) <= thresh2 ? 1 : 0;
        count = wave_sum(count);
        if (lane == 0) sCount[m] = count;
    }
}

// the sequential loop of RANSACPointSetRegistrator::run over this round's iterations, on ONE lane: slot by slot the best-model rule
// (good > max(maxGood, modelPoints - 1)) and RANSACUpdateNumIters; where the sampler stopped, its code (1: no subset, and no model at
// all if that was iteration 0; 2: the cap).  sNModels[slot] models at kPerSlot * slot.
template <int kDoubles, int kPerSlot, int kModelPoints>
__device__ __forceinline__ void replay_round(State &s, int n, double confidence, const double (*sModel)[kDoubles], const int *sNModels, const int *sCount,
                                             double *sBest)
{
    int iter = s.iter, niters = s.niters, maxGood = s.maxGood, stop = 0;
    const int drawn = s.drawn;
    for (int slot = 0;; slot++) {
        if (iter >= niters) break;
        if (slot == drawn) {  // the sampler stopped here (or the round is used up)
            if (s.stop == 2) { s.result = -2; stop = 1; }
            else if (s.stop == 1) { stop = 1; if (iter == 0) maxGood = 0; }
            break;
        }
        for (int m = 0; m < sNModels[slot]; m++) {
            const int good = sCount[kPerSlot * slot + m];
            if (good > max(maxGood, kModelPoints - 1)) {
                for (int k = 0; k < kDoubles; k++) sBest[k] = sModel[kPerSlot * slot + m][k];
                maxGood = good;
                niters = fm::update_num_iters(confidence, fm::dvd((double)(n - good), (double)n), niters, kModelPoints);
            }
        }
        iter++;
    }
    s.iter = iter; s.niters = niters; s.maxGood = maxGood;
    if (iter >= niters) stop = 1;
    s.stop = stop ? 3 : 0;
}

}  // namespace ransac
}  // namespace amos
