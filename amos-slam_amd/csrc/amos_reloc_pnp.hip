// amos_reloc_pnp.hip -- step 3 of Tracking::Relocalization's candidate loop (Tracking.cc:2650-2713): ORB-SLAM2's PnPsolver
// (src/PnPsolver.cc:120-458: constructor, SetRansacParameters, iterate, CheckInliers, Refine) for a batch of pairs (lost frame, candidate
// keyframe) on resident frames, and the loop of Tracking.cc:2704-2713 that turns vbInliers into the frame's matches and sFound.
// The arithmetic is amos_pnp_core.h (EPnP restated, parity with the reference's OpenCV-backed EPnP unpinned; the solver_* pieces), the
// block-wide EPnP of Refine amos_pnp_block.h (shared with k_pnp_ransac), the compaction amos_block.h; tests/reloc_pnp_restatement.py is
// the same in Python and the GPU tests hold the kernel to it bit for bit.
//   k_reloc_pnp_iterate  ONE WORK-GROUP PER PAIR (a batch of pairs is one launch), one PnPsolver::iterate call each.  The correspondences
//                  (features whose SearchByBoW match names a point without the skip bit) are compacted into LDS (21 B each).  The RANSAC runs
//                  in rounds of up to kRpRound drawn-ahead iterations: lane 0 runs the serial generator (every iteration consumes exactly
//                  four draws, so drawing ahead changes nothing; the state behind each iteration is kept, and the one behind the last
//                  iteration the reference would have run is carried); one group of sixteen lanes per hypothesis, two groups per wave, runs
//                  pnp::epnp_serial on its four points with its 12 x 12 MtM and eigenvectors in an LDS slab (the lanes of a group compute the
//                  same values and share the Jacobi's rotations: amos_pnp_block.h); all waves score the round's
//                  models over all correspondences (ballots: counts and inlier masks, no atomics); lane 0 replays the iterations in order
//                  and stops at the first one whose Refine is not known; the work-group runs that Refine (block_epnp over the best set,
//                  CheckInliers by all waves), remembers its outcome for as long as the best set stands, and the replay goes on.
//                  Between calls only the carried state lives: generator, counters, adjusted parameters, best and refined pose and
//                  inlier masks (by correspondence index: the inputs of a carried state must not change between its calls).
#include "amos_block.h"
#include "amos_match_core.h"
#include "amos_pnp_block.h"
#include "amos_projection_search.h"

#include <cmath>
#include <vector>

namespace amos {

constexpr int kRpThreads = 512, kRpWaves = kRpThreads / 64;
constexpr int kRpRound = 16, kRpPerWave = kRpRound / kRpWaves;
constexpr int kRpMax = pnp::kSolverMaxPoints, kRpWords = kRpMax / 32;
constexpr int kRpMaxIterations = 65536;
constexpr uint32_t kRpMagic = 0x506e5031u;

static_assert(sizeof(amos_reloc_pnp_params) == 64, "amos_reloc_pnp_params is 64 bytes");
static_assert(sizeof(amos_reloc_pnp_result) == 104, "amos_reloc_pnp_result is 104 bytes");
static_assert(kRpRound % kRpWaves == 0, "the hypotheses of a round are spread evenly over the waves");

struct RpState {  // the head of a pair's carried state; pnp::kEpnpScratch doubles per correspondence follow at kRpHeader
    uint64_t rng;
    uint32_t magic;
    int n, minInliers, maxIts, iterations, bestInliers, refineValid, refineOk, refinedInliers;
    float eps;
    float bestTcw[12], refinedTcw[12];
    uint32_t bestMask[kRpWords], refinedMask[kRpWords];
};
constexpr size_t kRpHeader = (sizeof(RpState) + 63) & ~(size_t)63;

inline size_t rp_state_bytes(int capacity)
{
    const size_t rows = (size_t)std::min(std::max(capacity, 1), kRpMax);
    return kRpHeader + ((rows * pnp::kEpnpScratch * sizeof(double) + 63) & ~(size_t)63);
}

struct RpPair {
    amos_reloc_pnp_params par;
    int frame, off0, off1, pad;
};

struct RpArgs {
    const amos_keypoint *kps;  // [frames][capacity]
    const int *counts;
    const amos_reloc_point *points;
    const int *bow;            // [pairs][capacity]
    const RpPair *pairs;
    uint8_t *state;
    size_t stateStride;
    amos_reloc_pnp_result *result;
    uint8_t *inlier;           // [pairs][capacity]
    int *match;                // [pairs][capacity]
    uint8_t *found;            // one per point
    float sigma2[AMOS_MAX_LEVELS];
    int capacity, nLevels;
};

enum { kRpRoundDone = 0, kRpNeedRefine = 1, kRpReturnRefined = 2, kRpFinished = 3 };

struct RpCtl {  // in LDS, written by one lane between barriers
    uint64_t rng;
    int minInliers, maxIts, iterations, bestInliers, refineValid, refineOk, refinedInliers;
    float eps;
    float bestTcw[12], refinedTcw[12];
    int remaining, cur, drawn, next, act;
};

__device__ __forceinline__ bool mask_bit(const uint32_t *w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }

__global__ __launch_bounds__(kRpThreads) void k_reloc_pnp_iterate(const RpArgs a)
{
    __shared__ float4 sP[kRpMax];     // (X, Y, Z, u) of the correspondences
    __shared__ float sV[kRpMax];      // v
    __shared__ uint8_t sOct[kRpMax];  // octave: the threshold is sMaxErr[octave]
    __shared__ uint16_t sIdx[kRpMax]; // Refine's points: the best set in ascending order
    __shared__ double sHM[kRpRound][144], sHE[kRpRound][144];  // per hypothesis: MtM and its eigenvectors
    __shared__ double sModel[kRpRound][12];
    __shared__ uint32_t sMask[kRpRound][kRpWords];
    __shared__ uint32_t sBestMask[kRpWords], sRefMask[kRpWords];
    __shared__ int sCount[kRpRound], sSub[kRpRound][4];
    __shared__ uint64_t sRngAfter[kRpRound];
    __shared__ float sMaxErr[AMOS_MAX_LEVELS];
    __shared__ EpnpShared sE;
    __shared__ RpCtl sC;
    __shared__ int sWave[kRpWaves];
    const int pair = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const RpPair &pr = a.pairs[pair];
    amos_reloc_pnp_result *res = a.result + pair;
    if (!pr.par.enabled) {  // the whole work-group: nothing but the record is written
        if (t == 0) {
            amos_reloc_pnp_result r = {};
            r.skipped = 1;
            *res = r;
        }
        return;
    }
    const int cap = a.capacity, cnt = min(max(a.counts[pr.frame], 0), cap), nPts = pr.off1 - pr.off0;
    const amos_keypoint *kps = a.kps + (size_t)pr.frame * cap;
    const int *bow = a.bow + (size_t)pair * cap;
    const amos_reloc_point *points = a.points + pr.off0;
    uint8_t *inlierOut = a.inlier + (size_t)pair * cap;
    int *matchOut = a.match + (size_t)pair * cap;
    RpState *S = reinterpret_cast<RpState *>(a.state + (size_t)pair * a.stateStride);
    double *scr = reinterpret_cast<double *>(a.state + (size_t)pair * a.stateStride + kRpHeader);

    // ---- the constructor's walk (PnPsolver.cc:136-158): correspondences in ascending feature order
    int bad = 0;
    auto selected = [&](int i) {
        const int j = bow[i];
        if (j < 0) return false;
        if (j >= nPts) { bad |= 2; return false; }
        if (points[j].flags & AMOS_RELOC_POINT_SKIP) return false;
        const int oct = kps[i].octave;
        if (oct < 0 || oct >= a.nLevels) { bad |= 1; return false; }
        return true;
    };
    const int n = block_compact<kRpThreads>(cnt, sWave, selected, [&](int i, int c) {
        if (c >= 0 && c < kRpMax) {
            const amos_keypoint k = kps[i];
            const float *p = points[bow[i]].pos;
            sP[c] = make_float4(p[0], p[1], p[2], k.x);
            sV[c] = k.y;
            sOct[c] = (uint8_t)k.octave;
        }
    });
    const int badOct = block_sum<kRpThreads>(bad & 1, sWave), badIdx = block_sum<kRpThreads>(bad & 2, sWave);
    int status = (badOct ? 1 : 0) | (badIdx ? 2 : 0);
    if (n > kRpMax) {  // more than k_pnp_ransac's limit: code -3, no output but the record
        if (t == 0) {
            amos_reloc_pnp_result r = {};
            r.code = -3; r.n_correspondences = n; r.status = status;
            *res = r;
        }
        return;
    }
    // ---- the carried state; reset: SetRansacParameters (PnPsolver.cc:181-230)
    const bool carried = !pr.par.reset && S->magic == kRpMagic && S->n == n && S->maxIts >= 1 && S->maxIts <= kRpMaxIterations;
    if (!pr.par.reset && !carried) status |= 4;  // the state is not one of these inputs: the call starts over
    if (t == 0) {
        if (carried) {
            sC.rng = S->rng; sC.minInliers = S->minInliers; sC.maxIts = S->maxIts; sC.iterations = S->iterations;
            sC.bestInliers = S->bestInliers; sC.refineValid = S->refineValid; sC.refineOk = S->refineOk; sC.refinedInliers = S->refinedInliers;
            sC.eps = S->eps;
            for (int k = 0; k < 12; k++) { sC.bestTcw[k] = S->bestTcw[k]; sC.refinedTcw[k] = S->refinedTcw[k]; }
        } else {
            pnp::solver_parameters(n, pr.par.probability, pr.par.min_inliers, pr.par.max_iterations, pr.par.epsilon, sC.minInliers, sC.maxIts, sC.eps);
            sC.rng = pr.par.seed; sC.iterations = 0; sC.bestInliers = 0; sC.refineValid = 0; sC.refineOk = 0; sC.refinedInliers = 0;
            for (int k = 0; k < 12; k++) { sC.bestTcw[k] = 0.f; sC.refinedTcw[k] = 0.f; }
        }
        const int left = sC.maxIts - sC.iterations;  // while (mnIterations < maxIts || nCurrentIterations < nIterations)
        sC.remaining = max(left, pr.par.n_iterations);
        sC.cur = 0;
        sC.act = kRpFinished;
    }
    if (t < kRpWords) {
        sBestMask[t] = carried ? S->bestMask[t] : 0u;
        sRefMask[t] = carried ? S->refinedMask[t] : 0u;
    }
    if (t < AMOS_MAX_LEVELS) sMaxErr[t] = pnp::fmul(a.sigma2[t], pr.par.th2);  // mvMaxError[i] = mvSigma2[i] * th2
    __syncthreads();
    const double fu = (double)pr.par.fx, fv = (double)pr.par.fy, uc = (double)pr.par.cx, vc = (double)pr.par.cy;
    const int minInliers = sC.minInliers, nWords = (n + 31) >> 5;
    auto inlier_of = [&](const double *M, int i) {
        const float4 P = sP[i];
        return pnp::solver_inlier(M, P.x, P.y, P.z, P.w, sV[i], fu, fv, uc, vc, sMaxErr[sOct[i]]);
    };

    int act = kRpFinished;
    if (n >= minInliers) {  // else bNoMore, no pose (PnPsolver.cc:246-250)
        for (;;) {
            // ---- draw the subsets of the next iterations (PnPsolver.cc:268-283)
            if (t == 0) {
                const int limit = min(kRpRound, sC.remaining);
                uint64_t rng = sC.rng;
                for (int slot = 0; slot < limit; slot++) {
                    int idx[4];
                    pnp::solver_draw4(rng, n, idx);
                    for (int i = 0; i < 4; i++) sSub[slot][i] = idx[i];
                    sRngAfter[slot] = rng;
                }
                sC.drawn = limit; sC.next = 0;
            }
            __syncthreads();
            const int drawn = sC.drawn;
            // ---- compute_pose on four points: hypothesis h on lane group h / kRpWaves of wave h % kRpWaves.  The sixteen lanes of a group
            // run the same solve on the same points (identical values, identical writes); inside it they share the 12 x 12 Jacobi's rotations
            const int group = lane / kJacobiGroup, h = group * kRpWaves + wv;
            if (group < kRpPerWave && h < drawn) {
                const int *sub = sSub[h];
                double alphaRows[4 * pnp::kEpnpScratch], Rt[12];
                pnp::epnp_serial<pnp::PixelDirect>(4, [&](int j, double *pw, float &u, float &v) {
                    const float4 P = sP[sub[j]];
                    pw[0] = P.x; pw[1] = P.y; pw[2] = P.z;
                    u = P.w; v = sV[sub[j]];
                }, fu, fv, uc, vc, alphaRows, sHM[h], sHE[h], Rt, Jacobi12Group{lane % kJacobiGroup});
                if (lane % kJacobiGroup == 0)
                    for (int k = 0; k < 12; k++) sModel[h][k] = Rt[k];
            }
            __syncthreads();
            // ---- CheckInliers of every model of the round: model m on wave m % kRpWaves, 64 correspondences per ballot
            for (int m = wv; m < drawn; m += kRpWaves) {
                double M[12];
#pragma unroll
                for (int k = 0; k < 12; k++) M[k] = sModel[m][k];
                int count = 0;
                for (int base = 0; base < n; base += 64) {
                    const int i = base + lane;
                    const unsigned long long b = __ballot(i < n && inlier_of(M, i));
                    count += (int)__popcll(b);
                    if (lane == 0) { sMask[m][base >> 5] = (uint32_t)b; sMask[m][(base >> 5) + 1] = (uint32_t)(b >> 32); }
                }
                if (lane == 0) sCount[m] = count;
            }
            __syncthreads();
            // ---- the sequential loop over the round's iterations, interrupted where a Refine has to run
            for (;;) {
                if (t == 0) {
                    int out = kRpRoundDone;
                    for (int slot = sC.next; slot < sC.drawn; slot++) {
                        sC.iterations++; sC.cur++; sC.remaining--;
                        sC.rng = sRngAfter[slot];
                        const int c = sCount[slot];
                        if (c < minInliers) continue;
                        if (c > sC.bestInliers) {
                            sC.bestInliers = c;
                            for (int w = 0; w < nWords; w++) sBestMask[w] = sMask[slot][w];
                            pnp::solver_tcw(sModel[slot], sC.bestTcw);
                            sC.refineValid = 0;
                        }
                        if (!sC.refineValid) { out = kRpNeedRefine; sC.next = slot + 1; break; }
                        if (sC.refineOk) { out = kRpReturnRefined; break; }
                    }
                    if (out == kRpRoundDone && sC.remaining <= 0) out = kRpFinished;
                    sC.act = out;
                }
                __syncthreads();
                act = sC.act;  // the same value in every thread: the loops' barriers stay uniform
                if (act != kRpNeedRefine) break;
                // ---- Refine (PnPsolver.cc:366-418): EPnP over the best set in ascending order, then CheckInliers
                const int m = block_compact<kRpThreads>(n, sWave, [&](int i) { return mask_bit(sBestMask, i); },
                                                        [&](int i, int c) { if (c >= 0) sIdx[c] = (uint16_t)i; });
                block_epnp<kRpThreads, pnp::PixelDirect>(sE, m, [&](int j, double *pw) {
                    const float4 P = sP[sIdx[j]];
                    pw[0] = P.x; pw[1] = P.y; pw[2] = P.z;
                }, [&](int j, float &u, float &v) { u = sP[sIdx[j]].w; v = sV[sIdx[j]]; }, fu, fv, uc, vc, scr);
                const int N = epnp_pick(sE);
                double M[12];
#pragma unroll
                for (int k = 0; k < 12; k++) M[k] = sE.Rt[N][k];
                int count = 0;
                for (int base = wv * 64; base < n; base += kRpThreads) {
                    const int i = base + lane;
                    const unsigned long long b = __ballot(i < n && inlier_of(M, i));
                    count += (int)__popcll(b);
                    if (lane == 0) { sRefMask[base >> 5] = (uint32_t)b; sRefMask[(base >> 5) + 1] = (uint32_t)(b >> 32); }
                }
                const int refined = block_sum<kRpThreads>(lane == 0 ? count : 0, sWave);
                if (t == 0) {
                    sC.refineValid = 1;
                    sC.refinedInliers = refined;
                    sC.refineOk = refined > minInliers ? 1 : 0;  // strict
                    pnp::solver_tcw(M, sC.refinedTcw);
                    if (sC.refineOk) sC.act = kRpReturnRefined;
                }
                __syncthreads();
                act = sC.act;
                if (act == kRpReturnRefined) break;
            }
            if (act != kRpRoundDone) break;
        }
    }
    __syncthreads();
    // ---- the end of iterate (PnPsolver.cc:343-362) and the loop of Tracking.cc:2704-2713
    const bool refinedPose = act == kRpReturnRefined;
    const bool noMore = !refinedPose && (n < minInliers || sC.iterations >= sC.maxIts);
    const bool bestPose = !refinedPose && n >= minInliers && noMore && sC.bestInliers >= minInliers;
    const bool hasPose = refinedPose || bestPose;
    const uint32_t *outMask = refinedPose ? sRefMask : sBestMask;
    if (hasPose && a.found)
        for (int j = t; j < nPts; j += kRpThreads) a.found[pr.off0 + j] = 0;
    __syncthreads();
    block_compact<kRpThreads>(cnt, sWave, selected, [&](int i, int c) {
        const bool in = hasPose && c >= 0 && mask_bit(outMask, c);
        inlierOut[i] = in ? 1 : 0;
        if (hasPose) {
            const int j = bow[i];
            matchOut[i] = in ? j : -1;
            if (in && a.found) a.found[pr.off0 + j] = 1;  // several features of one point write the same value
        }
    });
    for (int i = cnt + t; i < cap; i += kRpThreads) {
        inlierOut[i] = 0;
        if (hasPose) matchOut[i] = -1;
    }
    if (t < kRpWords) { S->bestMask[t] = sBestMask[t]; S->refinedMask[t] = sRefMask[t]; }
    if (t == 0) {
        S->rng = sC.rng; S->magic = kRpMagic; S->n = n; S->minInliers = sC.minInliers; S->maxIts = sC.maxIts; S->iterations = sC.iterations;
        S->bestInliers = sC.bestInliers; S->refineValid = sC.refineValid; S->refineOk = sC.refineOk; S->refinedInliers = sC.refinedInliers;
        S->eps = sC.eps;
        for (int k = 0; k < 12; k++) { S->bestTcw[k] = sC.bestTcw[k]; S->refinedTcw[k] = sC.refinedTcw[k]; }
        amos_reloc_pnp_result r = {};
        for (int k = 0; k < 12; k++) r.Tcw[k] = refinedPose ? sC.refinedTcw[k] : (bestPose ? sC.bestTcw[k] : 0.f);
        r.has_pose = hasPose ? 1 : 0; r.no_more = noMore ? 1 : 0; r.refined = refinedPose ? 1 : 0;
        r.n_inliers = refinedPose ? sC.refinedInliers : (bestPose ? sC.bestInliers : 0);
        r.n_correspondences = n; r.min_inliers = sC.minInliers; r.max_iterations = sC.maxIts;
        r.iterations = sC.iterations; r.iterations_call = sC.cur; r.best_inliers = sC.bestInliers; r.status = status;
        *res = r;
    }
}

}  // namespace amos

using namespace amos;

static bool rp_params_ok(const char *name, const amos_reloc_pnp_params &p, int k)
{
    const bool ok = std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.cx) && std::isfinite(p.cy) && p.probability > 0.0 && p.probability < 1.0 &&
                    std::isfinite(p.epsilon) && p.epsilon > 0.f && std::isfinite(p.th2) && p.th2 > 0.f && p.max_iterations >= 1 &&
                    p.max_iterations <= kRpMaxIterations && p.n_iterations >= 1 && p.n_iterations <= kRpMaxIterations;
    if (!ok)
        set_error("%s: pair %d: a camera that is not finite, a probability outside (0, 1), an epsilon or th2 that is not finite and positive, or a "
                  "max_iterations / n_iterations outside 1 .. %d", name, k, kRpMaxIterations);
    return ok;
}

extern "C" {

size_t amos_reloc_pnp_state_bytes(int capacity) { return rp_state_bytes(capacity); }

int amos_match_reloc_pnp_batch_device(amos_match *m, const amos_reloc_pnp *s)
{
    static const char *name = "amos_match_reloc_pnp_batch_device";
    if (!m || !s || !s->d_kps || !s->d_counts || !s->frame_of_pair || !s->point_off || !s->d_points || !s->d_bow_match || !s->level_sigma2 || !s->params ||
        !s->d_state || !s->d_result || !s->d_inlier || !s->d_match || s->n_pairs < 1 || s->n_frames < 1 || s->capacity < 1 || s->capacity > 65536 ||
        s->n_levels < 1 || s->n_levels > AMOS_MAX_LEVELS) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    if (s->point_off[0] < 0) { set_error("%s: point_off[0] < 0", name); return AMOS_ERR_INVALID; }
    for (int k = 0; k < s->n_pairs; k++) {
        if (s->frame_of_pair[k] < 0 || s->frame_of_pair[k] >= s->n_frames) { set_error("%s: frame_of_pair[%d] outside the frames", name, k); return AMOS_ERR_INVALID; }
        if (s->point_off[k + 1] < s->point_off[k]) { set_error("%s: point_off descends at %d", name, k); return AMOS_ERR_INVALID; }
        if (!rp_params_ok(name, s->params[k], k)) return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    int rc = grow(&m->dLocal, &m->capLocal, sizeof(RpPair) * (size_t)s->n_pairs);
    if (rc != AMOS_OK) return rc;
    std::vector<RpPair> pairs((size_t)s->n_pairs);
    for (int k = 0; k < s->n_pairs; k++) pairs[k] = RpPair{s->params[k], s->frame_of_pair[k], s->point_off[k], s->point_off[k + 1], 0};
    rc = upload_frames(m, pairs.data(), sizeof(RpPair) * pairs.size());
    if (rc != AMOS_OK) return rc;
    RpArgs a;
    a.kps = s->d_kps; a.counts = s->d_counts; a.points = s->d_points; a.bow = s->d_bow_match; a.pairs = (const RpPair *)m->dLocal;
    a.state = (uint8_t *)s->d_state; a.stateStride = rp_state_bytes(s->capacity);
    a.result = s->d_result; a.inlier = s->d_inlier; a.match = s->d_match; a.found = s->d_found;
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.sigma2[l] = l < s->n_levels ? s->level_sigma2[l] : 0.f;
    a.capacity = s->capacity; a.nLevels = s->n_levels;
    hipLaunchKernelGGL(k_reloc_pnp_iterate, dim3(s->n_pairs), dim3(kRpThreads), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_reloc_pnp(amos_match *m, const amos_keypoint *kps_un, int n, const int32_t *bow_match, const amos_reloc_point *points, int n_points,
                         const float *level_sigma2, int n_levels, const amos_reloc_pnp_params *params, void *state, amos_reloc_pnp_result *result,
                         uint8_t *inlier, int32_t *match, uint8_t *found)
{
    static const char *name = "amos_match_reloc_pnp";
    if (!m || !level_sigma2 || !params || !state || !result || n < 0 || n > 65536 || n_points < 0 || (n > 0 && (!kps_un || !bow_match || !inlier || !match)) ||
        (n_points > 0 && (!points || !found)) || n_levels < 1 || n_levels > AMOS_MAX_LEVELS) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    if (!rp_params_ok(name, *params, 0)) return AMOS_ERR_INVALID;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t cap = (size_t)std::max(n, 1), np1 = (size_t)std::max(n_points, 1);
    const size_t bytesState = rp_state_bytes((int)cap), bytesMatch = sizeof(int32_t) * cap;
    const size_t oInlier = align64(sizeof(amos_reloc_pnp_result)), oMatch = oInlier + align64(cap), oFound = oMatch + align64(bytesMatch),
                 oHead = oFound + align64(np1), oEnd = oHead + kRpHeader;
    int rc = stage_begin(m, cap * (sizeof(amos_keypoint) + 4) + np1 * sizeof(amos_reloc_point) + bytesState + 64 * 8 + oEnd);
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, oEnd);
    if (rc != AMOS_OK) return rc;
    const std::vector<uint8_t> zeros(std::max(cap * sizeof(amos_keypoint), sizeof(amos_reloc_point)), 0);  // an empty frame still hands valid arrays down
    const int32_t count = n, frameOfPair = 0, off[2] = {0, n_points};
    amos_reloc_pnp s;
    s.d_kps = stage_input<amos_keypoint>(m, n ? (const void *)kps_un : zeros.data(), sizeof(amos_keypoint) * cap);
    s.d_counts = stage_input<int32_t>(m, &count, sizeof(count));
    s.d_bow_match = stage_input<int32_t>(m, n ? (const void *)bow_match : zeros.data(), bytesMatch);
    s.d_points = stage_input<amos_reloc_point>(m, n_points ? (const void *)points : zeros.data(), sizeof(amos_reloc_point) * np1);
    s.d_state = stage_input<uint8_t>(m, state, kRpHeader);  // the head travels; the scratch rows behind it are the call's own
    (void)stage_take(m, bytesState - kRpHeader);
    s.frame_of_pair = &frameOfPair; s.point_off = off; s.level_sigma2 = level_sigma2; s.params = params;
    uint8_t *out = (uint8_t *)m->dOut;
    s.d_result = (amos_reloc_pnp_result *)out; s.d_inlier = out + oInlier; s.d_match = (int32_t *)(out + oMatch); s.d_found = out + oFound;
    s.n_frames = 1; s.n_pairs = 1; s.capacity = (int32_t)cap; s.n_levels = n_levels;
    if ((rc = stage_flush(m)) != AMOS_OK) return rc;
    AMOS_HIP_CHECK(hipMemsetAsync(out, 0, oHead, m->stream));  // a call without a pose leaves match and found unwritten: they come back as zeros
    if ((rc = amos_match_reloc_pnp_batch_device(m, &s)) != AMOS_OK) return rc;
    AMOS_HIP_CHECK(hipMemcpyAsync(out + oHead, s.d_state, kRpHeader, hipMemcpyDeviceToDevice, m->stream));
    uint8_t *h = m->hStage + stage_take(m, oEnd);
    AMOS_HIP_CHECK(hipMemcpyAsync(h, out, oEnd, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    std::memcpy(result, h, sizeof(amos_reloc_pnp_result));
    const bool pose = result->has_pose != 0;
    if (n) {
        std::memcpy(inlier, h + oInlier, (size_t)n);
        if (pose) std::memcpy(match, h + oMatch, sizeof(int32_t) * (size_t)n);
    }
    if (n_points && pose) std::memcpy(found, h + oFound, (size_t)n_points);
    if (result->code == 0 && !result->skipped) std::memcpy(state, h + oHead, kRpHeader);
    return AMOS_OK;
}

}  // extern "C"
