// amos_sim3.hip -- step 2 of LoopClosing::ComputeSim3's candidate loop (LoopClosing.cc:389-447): ORB-SLAM2's Sim3Solver
// (src/Sim3Solver.cc:48-523: constructor, SetRansacParameters, iterate, ComputeSim3, CheckInliers) for a batch of pairs (keyframe-1 slot,
// keyframe-2 slot) on resident keyframes, and the loop of LoopClosing.cc:440-447 that turns vbInliers into the row SearchBySim3 starts
// from.  The arithmetic is amos_sim3_core.h (Horn's closed form restated, parity with the reference's OpenCV-backed arithmetic unpinned),
// the compaction amos_block.h; tests/sim3_restatement.py is the same in Python and the GPU tests hold the kernel to it bit for bit.
//   k_sim3_iterate  ONE WORK-GROUP PER PAIR (a batch of pairs is one launch), one Sim3Solver::iterate call each.  The correspondences are
//                  compacted into LDS in ascending i1 (48 B each: X3Dc1, X3Dc2, the two image points, the two bounds; 2048 of them are
//                  96 KB beside 9 KB of hypotheses).  The RANSAC runs in rounds of up to kS3Round drawn-ahead iterations (kS3FirstRound in a call's first): lane 0 steps
//                  the serial generator (every iteration consumes exactly three draws, so drawing ahead changes nothing; the state behind
//                  each iteration is kept, and the one behind the last iteration the reference would have run is carried); every thread
//                  of the first wave turns its three outputs into indices and solves ONE hypothesis (sim3::sim3_horn, in registers); the waves score
//                  the round's hypotheses over all correspondences (ballots: counts only, no atomics); lane 0 replays the iterations in
//                  order (the >= best update, the > minInliers return: iterations behind the return leave no trace); the inlier mask of
//                  the round's last best hypothesis is then computed once by all waves.
//                  Between calls only the carried state lives: generator, counters, adjusted parameters, the best Sim3 and its inlier
//                  mask (by correspondence index: the inputs of a carried state must not change between its calls).
#include "amos_block.h"
#include "amos_match_core.h"
#include "amos_projection_search.h"
#include "amos_sim3_core.h"

#include <cmath>
#include <vector>

namespace amos {

constexpr int kS3Threads = 256, kS3Waves = kS3Threads / 64;
constexpr int kS3Round = 64;  // one wave solves a round's hypotheses; the defaults (0.99, 20, 300) adjust to 123 iterations at 60 correspondences
constexpr int kS3FirstRound = 8;  // a call's first round is short: with the loop closer's inlier shares the return comes within a few iterations
constexpr int kS3Max = sim3::kMaxCorrespondences, kS3Words = kS3Max / 32;
constexpr int kS3MaxIterations = 65536;
constexpr int kS3HypWords = 34;  // R 9, t 3, s 1, sR 9, sRi 9, ti 3
constexpr uint32_t kS3Magic = 0x53696d33u;

static_assert(sizeof(amos_sim3_point) == 16 && sizeof(amos_sim3_camera) == 64, "amos_sim3_point is 16 bytes, amos_sim3_camera 64");
static_assert(sizeof(amos_sim3_params) == 40 && sizeof(amos_sim3_result) == 160, "amos_sim3_params is 40 bytes, amos_sim3_result 160");
static_assert(kS3Max % 64 == 0, "a ballot covers 64 correspondences");

struct S3State {  // a pair's carried state
    uint64_t rng;
    uint32_t magic;
    int n, minInliers, fixScale, maxIts, iterations, bestInliers;
    float R[9], t[3], s, T12[16];
    uint32_t bestMask[kS3Words];
};
constexpr size_t kS3StateBytes = (sizeof(S3State) + 63) & ~(size_t)63;

struct S3Args {
    const amos_keypoint *kps;  // [frames][capacity]
    const int *counts;
    const amos_sim3_point *points;
    const amos_sim3_camera *cameras;  // [frames], uploaded by the call
    const amos_sim3_params *params;   // [pairs], uploaded by the call
    const int *pairs1, *pairs2;
    const int *match12;  // [pairs][capacity]
    uint8_t *state;
    amos_sim3_result *result;
    uint8_t *inlier;  // [pairs][capacity]
    int *matchOut;    // [pairs][capacity]
    float sigma2[AMOS_MAX_LEVELS];
    int capacity, nLevels, nFrames;
};

enum { kS3RoundDone = 0, kS3Return = 1, kS3Finished = 2 };

struct S3Ctl {  // in LDS, written by one lane between barriers
    uint64_t rng;
    int minInliers, fixScale, maxIts, iterations, bestInliers;
    float R[9], t[3], s, T12[16];
    int cur, drawn, bestSlot, act;
};

__global__ __launch_bounds__(kS3Threads) void k_sim3_iterate(const S3Args a)
{
    __shared__ float4 sA[kS3Max];  // X3Dc1, mvP1im1.x
    __shared__ float4 sB[kS3Max];  // X3Dc2, mvP2im2.x
    __shared__ float4 sE[kS3Max];  // mvP1im1.y, mvP2im2.y, mvnMaxError1, mvnMaxError2
    __shared__ float sH[kS3HypWords][kS3Round];
    __shared__ int sDeg[kS3Round], sCount[kS3Round];
    __shared__ uint32_t sRaw[kS3Round * 3];
    __shared__ uint64_t sRngAfter[kS3Round];
    __shared__ uint32_t sBestMask[kS3Words];
    __shared__ float sMaxErr[AMOS_MAX_LEVELS];
    __shared__ S3Ctl sC;
    __shared__ int sWave[kS3Waves];
    const int pair = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const amos_sim3_params par = a.params[pair];
    amos_sim3_result *res = a.result + pair;
    const int f1 = a.pairs1[pair], f2 = a.pairs2[pair];
    const bool badSlot = f1 < 0 || f1 >= a.nFrames || f2 < 0 || f2 >= a.nFrames;
    if (!par.enabled || badSlot) {  // the whole work-group: nothing but the record is written
        if (t == 0) {
            amos_sim3_result r = {};
            if (!par.enabled) r.skipped = 1;
            else r.code = -4;
            *res = r;
        }
        return;
    }
    const int cap = a.capacity, cnt1 = min(max(a.counts[f1], 0), cap), cnt2 = min(max(a.counts[f2], 0), cap);
    const amos_keypoint *kps1 = a.kps + (size_t)f1 * cap, *kps2 = a.kps + (size_t)f2 * cap;
    const amos_sim3_point *pts1 = a.points + (size_t)f1 * cap, *pts2 = a.points + (size_t)f2 * cap;
    const amos_sim3_camera cam1 = a.cameras[f1], cam2 = a.cameras[f2];
    const int *m12 = a.match12 + (size_t)pair * cap;
    uint8_t *inlierOut = a.inlier + (size_t)pair * cap;
    int *matchOut = a.matchOut + (size_t)pair * cap;
    S3State *S = reinterpret_cast<S3State *>(a.state + (size_t)pair * kS3StateBytes);
    const float K1[4] = {cam1.fx, cam1.fy, cam1.cx, cam1.cy}, K2[4] = {cam2.fx, cam2.fy, cam2.cx, cam2.cy};

    if (t < AMOS_MAX_LEVELS) sMaxErr[t] = sim3::max_error(a.sigma2[t]);
    __syncthreads();
    // ---- the constructor's walk (Sim3Solver.cc:78-127): correspondences in ascending i1
    int bad = 0;
    auto selected = [&](int i) {
        const int j = m12[i];
        if (j < 0) return false;
        if (j >= cnt2) { bad |= 2; return false; }
        if ((pts1[i].flags & AMOS_SIM3_POINT_SKIP) || (pts2[j].flags & AMOS_SIM3_POINT_SKIP)) return false;
        const int o1 = kps1[i].octave, o2 = kps2[j].octave;
        if (o1 < 0 || o1 >= a.nLevels || o2 < 0 || o2 >= a.nLevels) { bad |= 1; return false; }
        return true;
    };
    const int n = block_compact<kS3Threads>(cnt1, sWave, selected, [&](int i, int c) {
        if (c >= 0 && c < kS3Max) {
            const int j = m12[i];
            float X1[3], X2[3], u1, v1, u2, v2;
            sim3::to_camera(cam1.Rcw, cam1.tcw, pts1[i].pos, X1);
            sim3::to_camera(cam2.Rcw, cam2.tcw, pts2[j].pos, X2);
            sim3::to_image(X1[0], X1[1], X1[2], K1[0], K1[1], K1[2], K1[3], u1, v1);
            sim3::to_image(X2[0], X2[1], X2[2], K2[0], K2[1], K2[2], K2[3], u2, v2);
            sA[c] = make_float4(X1[0], X1[1], X1[2], u1);
            sB[c] = make_float4(X2[0], X2[1], X2[2], u2);
            sE[c] = make_float4(v1, v2, sMaxErr[kps1[i].octave], sMaxErr[kps2[j].octave]);
        }
    });
    const int badOct = block_sum<kS3Threads>(bad & 1, sWave), badIdx = block_sum<kS3Threads>(bad & 2, sWave);
    int status = (badOct ? 1 : 0) | (badIdx ? 2 : 0);
    if (n > kS3Max) {  // code -3, no output but the record
        if (t == 0) {
            amos_sim3_result r = {};
            r.code = -3; r.n_correspondences = n; r.status = status;
            *res = r;
        }
        return;
    }
    // ---- the carried state (a reset does not read it); reset: SetRansacParameters (Sim3Solver.cc:143-196)
    bool carried = false;
    if (!par.reset) {
        carried = S->magic == kS3Magic && S->n == n && S->minInliers >= 3 && S->maxIts >= 1 && S->maxIts <= kS3MaxIterations;
        if (!carried) status |= 4;  // the state is not one of these inputs: the call starts over
    }
    if (t == 0) {
        if (carried) {
            sC.rng = S->rng; sC.minInliers = S->minInliers; sC.fixScale = S->fixScale; sC.maxIts = S->maxIts; sC.iterations = S->iterations;
            sC.bestInliers = S->bestInliers; sC.s = S->s;
            for (int k = 0; k < 9; k++) sC.R[k] = S->R[k];
            for (int k = 0; k < 3; k++) sC.t[k] = S->t[k];
            for (int k = 0; k < 16; k++) sC.T12[k] = S->T12[k];
        } else {
            sC.rng = par.seed; sC.minInliers = par.min_inliers; sC.fixScale = par.fix_scale ? 1 : 0;
            sC.maxIts = sim3::sim3_parameters(n, par.probability, par.min_inliers, par.max_iterations);
            sC.iterations = 0; sC.bestInliers = 0; sC.s = 0.f;
            for (int k = 0; k < 9; k++) sC.R[k] = 0.f;
            for (int k = 0; k < 3; k++) sC.t[k] = 0.f;
            for (int k = 0; k < 16; k++) sC.T12[k] = 0.f;
        }
        sC.cur = 0; sC.drawn = 0; sC.bestSlot = -1; sC.act = kS3Finished;
    }
    if (t < kS3Words) sBestMask[t] = carried ? S->bestMask[t] : 0u;
    __syncthreads();
    const int minInliers = sC.minInliers;
    const bool fixScale = sC.fixScale != 0;
    auto hypothesis_at = [&](int m, sim3::Hypothesis &h) {
#pragma unroll
        for (int k = 0; k < 9; k++) { h.R[k] = sH[k][m]; h.sR[k] = sH[13 + k][m]; h.sRi[k] = sH[22 + k][m]; }
#pragma unroll
        for (int k = 0; k < 3; k++) { h.t[k] = sH[9 + k][m]; h.ti[k] = sH[31 + k][m]; }
        h.s = sH[12][m];
        h.degenerate = sDeg[m];
    };
    auto inlier_of = [&](const sim3::Hypothesis &h, int i) {
        const float4 A = sA[i], B = sB[i], E = sE[i];
        const sim3::Correspondence c = {{A.x, A.y, A.z}, {B.x, B.y, B.z}, {A.w, E.x}, {B.w, E.y}, E.z, E.w};
        return sim3::sim3_inlier(h, c, K1, K2);
    };

    int act = kS3Finished;
    if (n >= minInliers) {  // else bNoMore, no Sim3, nothing drawn (Sim3Solver.cc:206-210)
        for (;;) {
            // ---- the generator's outputs for the next iterations (Sim3Solver.cc:228-249: three draws each)
            if (t == 0) {
                const int left = min(sC.maxIts - sC.iterations, par.n_iterations - sC.cur);  // mnIterations < maxIts && nCurrentIterations < nIterations
                const int limit = max(min(sC.cur == 0 ? kS3FirstRound : kS3Round, left), 0);
                uint64_t rng = sC.rng;
                for (int slot = 0; slot < limit; slot++) {
                    for (int k = 0; k < 3; k++) sRaw[3 * slot + k] = fm::rng_next(rng);
                    sRngAfter[slot] = rng;
                }
                sC.drawn = limit; sC.bestSlot = -1;
            }
            __syncthreads();
            const int drawn = sC.drawn;  // the same value in every thread: the barriers below stay uniform
            if (drawn == 0) break;
            // ---- ComputeSim3 on three correspondences: hypothesis t on thread t
            if (t < drawn) {
                int idx[3], k3 = 3 * t;
                sim3::sim3_draw3_of([&]() { return sRaw[k3++]; }, n, idx);
                float P1[3][3], P2[3][3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float4 A = sA[idx[c]], B = sB[idx[c]];
                    P1[0][c] = A.x; P1[1][c] = A.y; P1[2][c] = A.z;
                    P2[0][c] = B.x; P2[1][c] = B.y; P2[2][c] = B.z;
                }
                sim3::Hypothesis h;
                sim3::sim3_horn(P1, P2, fixScale, h);
#pragma unroll
                for (int k = 0; k < 9; k++) { sH[k][t] = h.R[k]; sH[13 + k][t] = h.sR[k]; sH[22 + k][t] = h.sRi[k]; }
#pragma unroll
                for (int k = 0; k < 3; k++) { sH[9 + k][t] = h.t[k]; sH[31 + k][t] = h.ti[k]; }
                sH[12][t] = h.s;
                sDeg[t] = h.degenerate;
            }
            __syncthreads();
            // ---- CheckInliers of every hypothesis of the round: hypothesis m on wave m % kS3Waves, 64 correspondences per ballot
            for (int m = wv; m < drawn; m += kS3Waves) {
                sim3::Hypothesis h;
                hypothesis_at(m, h);
                int count = 0;
                for (int base = 0; base < n; base += 64) {
                    const int i = base + lane;
                    count += (int)__popcll(__ballot(i < n && inlier_of(h, i)));
                }
                if (lane == 0) sCount[m] = count;
            }
            __syncthreads();
            // ---- the sequential loop over the round's iterations (Sim3Solver.cc:223-278)
            if (t == 0) {
                int out = kS3RoundDone, bestSlot = -1;
                for (int slot = 0; slot < drawn; slot++) {
                    sC.iterations++; sC.cur++;
                    sC.rng = sRngAfter[slot];
                    const int c = sCount[slot];
                    if (c >= sC.bestInliers) {
                        sC.bestInliers = c;
                        bestSlot = slot;
                        if (c > minInliers) { out = kS3Return; break; }  // strict
                    }
                }
                if (out == kS3RoundDone && (sC.iterations >= sC.maxIts || sC.cur >= par.n_iterations)) out = kS3Finished;
                if (bestSlot >= 0) {
                    sim3::Hypothesis h;
                    hypothesis_at(bestSlot, h);
                    for (int k = 0; k < 9; k++) sC.R[k] = h.R[k];
                    for (int k = 0; k < 3; k++) sC.t[k] = h.t[k];
                    sC.s = h.s;
                    sim3::sim3_T12(h, sC.T12);
                }
                sC.bestSlot = bestSlot; sC.act = out;
            }
            __syncthreads();
            act = sC.act;
            const int bestSlot = sC.bestSlot;
            if (bestSlot >= 0) {  // mvbBestInliers = mvbInliersi of the round's last best iteration
                sim3::Hypothesis h;
                hypothesis_at(bestSlot, h);
                for (int base = wv * 64; base < n; base += kS3Threads) {
                    const int i = base + lane;
                    const unsigned long long b = __ballot(i < n && inlier_of(h, i));
                    if (lane == 0) { sBestMask[base >> 5] = (uint32_t)b; sBestMask[(base >> 5) + 1] = (uint32_t)(b >> 32); }
                }
            }
            __syncthreads();
            if (act != kS3RoundDone) break;
        }
    }
    __syncthreads();
    // ---- the end of iterate (Sim3Solver.cc:267-284) and the loop of LoopClosing.cc:440-447
    const bool hasSim3 = act == kS3Return;
    const bool noMore = !hasSim3 && (n < minInliers || sC.iterations >= sC.maxIts);
    block_compact<kS3Threads>(cnt1, sWave, selected, [&](int i, int c) {
        const bool in = hasSim3 && c >= 0 && ((sBestMask[c >> 5] >> (c & 31)) & 1u);
        inlierOut[i] = in ? 1 : 0;
        if (hasSim3) matchOut[i] = in ? m12[i] : -1;
    });
    for (int i = cnt1 + t; i < cap; i += kS3Threads) {
        inlierOut[i] = 0;
        if (hasSim3) matchOut[i] = -1;
    }
    if (t < kS3Words) S->bestMask[t] = sBestMask[t];
    if (t == 0) {
        S->rng = sC.rng; S->magic = kS3Magic; S->n = n; S->minInliers = sC.minInliers; S->fixScale = sC.fixScale; S->maxIts = sC.maxIts;
        S->iterations = sC.iterations; S->bestInliers = sC.bestInliers; S->s = sC.s;
        for (int k = 0; k < 9; k++) S->R[k] = sC.R[k];
        for (int k = 0; k < 3; k++) S->t[k] = sC.t[k];
        for (int k = 0; k < 16; k++) S->T12[k] = sC.T12[k];
        amos_sim3_result r = {};
        if (hasSim3) {
            for (int k = 0; k < 9; k++) r.R12[k] = sC.R[k];
            for (int k = 0; k < 3; k++) r.t12[k] = sC.t[k];
            r.s12 = sC.s;
            for (int k = 0; k < 16; k++) r.T12[k] = sC.T12[k];
            r.n_inliers = sC.bestInliers;
        }
        r.has_sim3 = hasSim3 ? 1 : 0; r.no_more = noMore ? 1 : 0;
        r.n_correspondences = n; r.max_iterations = sC.maxIts;
        r.iterations = sC.iterations; r.iterations_call = sC.cur; r.best_inliers = sC.bestInliers; r.status = status;
        *res = r;
    }
}

}  // namespace amos

using namespace amos;

static bool s3_params_ok(const char *name, const amos_sim3_params &p, int k)
{
    const bool ok = p.probability > 0.0 && p.probability < 1.0 && p.min_inliers >= 3 && p.max_iterations >= 1 && p.max_iterations <= kS3MaxIterations &&
                    p.n_iterations >= 1 && p.n_iterations <= kS3MaxIterations;
    if (!ok)
        set_error("%s: pair %d: a probability outside (0, 1), min_inliers < 3, or a max_iterations / n_iterations outside 1 .. %d", name, k,
                  kS3MaxIterations);
    return ok;
}

static bool s3_camera_ok(const char *name, const amos_sim3_camera &c, int k)
{
    bool ok = std::isfinite(c.fx) && std::isfinite(c.fy) && std::isfinite(c.cx) && std::isfinite(c.cy);
    for (int i = 0; i < 9; i++) ok = ok && std::isfinite(c.Rcw[i]);
    for (int i = 0; i < 3; i++) ok = ok && std::isfinite(c.tcw[i]);
    if (!ok) set_error("%s: camera %d is not finite", name, k);
    return ok;
}

extern "C" {

size_t amos_sim3_state_bytes(int capacity)
{
    (void)capacity;  // the best set is a mask over the 2048 correspondences a solver may hold
    return kS3StateBytes;
}

int amos_match_sim3_batch_device(amos_match *m, const amos_sim3 *s)
{
    static const char *name = "amos_match_sim3_batch_device";
    if (!m || !s || !s->d_kps || !s->d_counts || !s->d_points || !s->cameras || !s->d_pairs_1 || !s->d_pairs_2 || !s->d_match12 || !s->level_sigma2 ||
        !s->params || !s->d_state || !s->d_result || !s->d_inlier || !s->d_match_out || s->n_pairs < 1 || s->n_frames < 1 || s->capacity < 1 ||
        s->capacity > 65536 || s->n_levels < 1 || s->n_levels > AMOS_MAX_LEVELS) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    if ((const void *)s->d_match_out == (const void *)s->d_match12) { set_error("%s: d_match_out is d_match12", name); return AMOS_ERR_INVALID; }
    for (int k = 0; k < s->n_frames; k++)
        if (!s3_camera_ok(name, s->cameras[k], k)) return AMOS_ERR_INVALID;
    for (int k = 0; k < s->n_pairs; k++)
        if (!s3_params_ok(name, s->params[k], k)) return AMOS_ERR_INVALID;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t bytesPar = align64(sizeof(amos_sim3_params) * (size_t)s->n_pairs), bytesCam = sizeof(amos_sim3_camera) * (size_t)s->n_frames;
    int rc = grow(&m->dLocal, &m->capLocal, bytesPar + bytesCam);
    if (rc != AMOS_OK) return rc;
    std::vector<uint8_t> host(bytesPar + bytesCam, 0);
    std::memcpy(host.data(), s->params, sizeof(amos_sim3_params) * (size_t)s->n_pairs);
    std::memcpy(host.data() + bytesPar, s->cameras, bytesCam);
    rc = upload_frames(m, host.data(), host.size());
    if (rc != AMOS_OK) return rc;
    S3Args a;
    a.kps = s->d_kps; a.counts = s->d_counts; a.points = s->d_points;
    a.params = (const amos_sim3_params *)m->dLocal; a.cameras = (const amos_sim3_camera *)(m->dLocal + bytesPar);
    a.pairs1 = s->d_pairs_1; a.pairs2 = s->d_pairs_2; a.match12 = s->d_match12;
    a.state = (uint8_t *)s->d_state; a.result = s->d_result; a.inlier = s->d_inlier; a.matchOut = s->d_match_out;
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.sigma2[l] = l < s->n_levels ? s->level_sigma2[l] : 0.f;
    a.capacity = s->capacity; a.nLevels = s->n_levels; a.nFrames = s->n_frames;
    hipLaunchKernelGGL(k_sim3_iterate, dim3(s->n_pairs), dim3(kS3Threads), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_sim3(amos_match *m, const amos_keypoint *kps1, const amos_sim3_point *points1, int n1, const amos_keypoint *kps2,
                    const amos_sim3_point *points2, int n2, const amos_sim3_camera *cameras, const int32_t *match12, const float *level_sigma2,
                    int n_levels, const amos_sim3_params *params, void *state, amos_sim3_result *result, uint8_t *inlier, int32_t *match_out)
{
    static const char *name = "amos_match_sim3";
    if (!m || !cameras || !level_sigma2 || !params || !state || !result || n1 < 0 || n1 > 65536 || n2 < 0 || n2 > 65536 ||
        (n1 > 0 && (!kps1 || !points1 || !match12 || !inlier || !match_out)) || (n2 > 0 && (!kps2 || !points2)) || n_levels < 1 ||
        n_levels > AMOS_MAX_LEVELS) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    if (!s3_params_ok(name, *params, 0) || !s3_camera_ok(name, cameras[0], 0) || !s3_camera_ok(name, cameras[1], 1)) return AMOS_ERR_INVALID;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t cap = (size_t)std::max(std::max(n1, n2), 1);
    const size_t bytesKps = sizeof(amos_keypoint) * cap, bytesPts = sizeof(amos_sim3_point) * cap, bytesMatch = sizeof(int32_t) * cap;
    const size_t oInlier = align64(sizeof(amos_sim3_result)), oMatch = oInlier + align64(cap), oState = oMatch + align64(bytesMatch),
                 oEnd = oState + kS3StateBytes;
    int rc = stage_begin(m, 2 * (bytesKps + bytesPts) + bytesMatch + kS3StateBytes + 64 * 10 + oEnd);
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, oEnd);
    if (rc != AMOS_OK) return rc;
    const int32_t counts[2] = {n1, n2}, slot1 = 0, slot2 = 1;
    amos_sim3 s;
    // the two keyframes are slots 0 and 1 of [2][cap] arrays (an empty keyframe still hands valid arrays down)
    std::vector<uint8_t> both(2 * std::max(bytesKps, bytesPts), 0);
    if (n1) std::memcpy(both.data(), kps1, sizeof(amos_keypoint) * (size_t)n1);
    if (n2) std::memcpy(both.data() + bytesKps, kps2, sizeof(amos_keypoint) * (size_t)n2);
    s.d_kps = stage_input<amos_keypoint>(m, both.data(), 2 * bytesKps);
    std::fill(both.begin(), both.end(), 0);
    if (n1) std::memcpy(both.data(), points1, sizeof(amos_sim3_point) * (size_t)n1);
    if (n2) std::memcpy(both.data() + bytesPts, points2, sizeof(amos_sim3_point) * (size_t)n2);
    s.d_points = stage_input<amos_sim3_point>(m, both.data(), 2 * bytesPts);
    s.d_counts = stage_input<int32_t>(m, counts, sizeof(counts));
    s.d_pairs_1 = stage_input<int32_t>(m, &slot1, sizeof(slot1));
    s.d_pairs_2 = stage_input<int32_t>(m, &slot2, sizeof(slot2));
    std::vector<int32_t> row(cap, -1);  // the row is capacity entries long
    if (n1) std::memcpy(row.data(), match12, sizeof(int32_t) * (size_t)n1);
    s.d_match12 = stage_input<int32_t>(m, row.data(), bytesMatch);
    s.d_state = stage_input<uint8_t>(m, state, kS3StateBytes);
    s.cameras = cameras; s.level_sigma2 = level_sigma2; s.params = params;
    uint8_t *out = (uint8_t *)m->dOut;
    s.d_result = (amos_sim3_result *)out; s.d_inlier = out + oInlier; s.d_match_out = (int32_t *)(out + oMatch);
    s.n_frames = 2; s.n_pairs = 1; s.capacity = (int32_t)cap; s.n_levels = n_levels;
    if ((rc = stage_flush(m)) != AMOS_OK) return rc;
    AMOS_HIP_CHECK(hipMemsetAsync(out, 0, oState, m->stream));  // a call without a Sim3 leaves match_out unwritten: it comes back as zeros
    if ((rc = amos_match_sim3_batch_device(m, &s)) != AMOS_OK) return rc;
    AMOS_HIP_CHECK(hipMemcpyAsync(out + oState, s.d_state, kS3StateBytes, hipMemcpyDeviceToDevice, m->stream));
    uint8_t *h = m->hStage + stage_take(m, oEnd);
    AMOS_HIP_CHECK(hipMemcpyAsync(h, out, oEnd, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    std::memcpy(result, h, sizeof(amos_sim3_result));
    if (n1) {
        std::memcpy(inlier, h + oInlier, (size_t)n1);
        if (result->has_sim3) std::memcpy(match_out, h + oMatch, sizeof(int32_t) * (size_t)n1);
    }
    if (result->code == 0 && !result->skipped) std::memcpy(state, h + oState, kS3StateBytes);
    return AMOS_OK;
}

}  // extern "C"
