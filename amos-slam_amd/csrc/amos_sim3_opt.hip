// amos_sim3_opt.hip -- step 4 of LoopClosing::ComputeSim3's candidate loop (LoopClosing.cc:461): Optimizer::OptimizeSim3
// (Optimizer.cc:1364-1590) for a batch of pairs of resident keyframes, behind amos_sim3.hip and amos_sim3_search.hip, whose result records
// and rows it reads in place: ONE launch, k_sim3_optimize, one work-group of so::kThreads per pair, built like k_pose_optimize
// (amos_pose.hip).  The prologue compacts the pair's correspondences (ascending keyframe-1 feature) into the handle's workspace; both
// optimisations, their Levenberg iterations and trials run inside the kernel.  Lanes 0 .. 13 make the 14 updates Sim3(+-delta e_d) of
// the numeric Jacobian once (one each) and apply them per linearisation: the 14 perturbed estimates depend on the estimate alone and lie in
// LDS with their inverses; every thread sums its correspondences c = t, t + kThreads, ... into its column of partials in LDS; the partials
// are folded in the fixed order of po::tree_sum by shuffles and one LDS exchange; thread 0 owns the Levenberg state (po::LmT<7, so::Pose>, in LDS), solves the 7 x 7 system and leaves the next estimate in LDS for
// all.  Every loop decision is read from LDS by all threads, so the barriers stay uniform.  No atomics, nothing to zero between calls.
// The arithmetic is defined in amos_sim3_opt_core.h; include/amos_frontend.h, "loop-closing Sim3 optimisation".
#include "amos_block.h"
#include "amos_match_core.h"
#include "amos_projection_search.h"  // align64, upload_frames
#include "amos_sim3_core.h"          // sim3::to_camera
#include "amos_sim3_opt_core.h"

#include <cmath>
#include <vector>

namespace amos {

static_assert(sizeof(amos_sim3_opt_pair) == 64, "amos_sim3_opt_pair is 64 bytes (include/amos_frontend.h)");
static_assert(sizeof(amos_sim3_opt_result) == 256 && sizeof(so::Out) == 256, "amos_sim3_opt_result is so::Out: 256 bytes");
static_assert(offsetof(amos_sim3_opt_result, R12) == 96 && offsetof(amos_sim3_opt_result, n_correspondences) == 212, "amos_sim3_opt_result's layout");
static_assert(sizeof(so::Corr) == 56, "so::Corr is 56 bytes");
static_assert(offsetof(amos_sim3_result, t12) == 36 && offsetof(amos_sim3_result, s12) == 48, "R12, t12, s12 are the solver result's first 13 floats");

struct S3OptArgs {
    const amos_keypoint *kps;           // [frames][capacity]
    const int *counts;
    const amos_sim3_point *points;      // [frames][capacity]
    const amos_sim3_camera *cameras;    // [frames], uploaded by the call
    const amos_sim3_opt_pair *pairs;    // [pairs], uploaded by the call
    const amos_sim3_result *sim3;       // [pairs] or null
    const int *pairs1, *pairs2;
    const int *matchIn;                 // [pairs][capacity]
    int *matchOut;                      // [pairs][capacity]
    amos_sim3_opt_result *result;
    so::Corr *corrs;                    // workspace [pairs][capacity]
    uint8_t *level;                     // workspace [pairs][capacity]: 1 = the correspondence left the problem
    float invSigma2[AMOS_MAX_LEVELS];
    int capacity, nLevels, nFrames;
};

// the fold of po::tree_sum inside one wave: lane i < s takes p[i] + p[i + s] for s = 32 .. 1 (addition commutes, so the xor partner serves)
__device__ __forceinline__ double s3o_wave_fold(double v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = so::add(v, __shfl_xor(v, s, 64));
    return v;
}

// grid = pairs, block = so::kThreads
__global__ __launch_bounds__(so::kThreads) void k_sim3_optimize(const S3OptArgs a)
{
    constexpr int kT = so::kThreads, kWaves = kT / 64;
    __shared__ po::LmT<so::kDim, so::Pose> lm;
    __shared__ so::Pose sInit;
    __shared__ so::Update sUpd[2 * so::kDim];  // the 14 updates of the numeric Jacobian: made once
    __shared__ so::Pose sPert[2 * so::kDim];    // the estimate behind each of them: made per linearisation
    __shared__ so::Cams sCams;
    __shared__ so::Out sOut;
    __shared__ double sAcc[so::kSums][kT];
    __shared__ double sPart[kWaves][so::kSums];
    __shared__ double sSums[so::kSums];
    __shared__ int sWave[kWaves];
    __shared__ int sAct;
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int f1 = a.pairs1[p], f2 = a.pairs2[p];
    const amos_sim3_opt_pair &pr = a.pairs[p];
    // ---- (uniform) a slot outside the frames, a skipped pair: the record alone
    int why = 0;
    const float *R12 = pr.R12, *t12 = pr.t12;
    float s12 = pr.s12;
    if (f1 < 0 || f1 >= a.nFrames || f2 < 0 || f2 >= a.nFrames) why = -4;
    else if (!pr.enabled) why = 1;
    else if (a.sim3) {
        const amos_sim3_result &r = a.sim3[p];
        if (!r.has_sim3 || r.code != 0) why = 1;
        R12 = r.R12; t12 = r.t12; s12 = r.s12;
    }
    if (why != 0) {
        if (t == 0) {
            so::out_zero(sOut);
            if (why == 1) sOut.skipped = 1;
            else sOut.code = why;
            a.result[p] = *reinterpret_cast<const amos_sim3_opt_result *>(&sOut);
        }
        return;
    }
    const int cap = a.capacity, n1 = min(max(a.counts[f1], 0), cap), n2 = min(max(a.counts[f2], 0), cap);
    const size_t row = (size_t)p * cap;
    const amos_keypoint *kps1 = a.kps + (size_t)f1 * cap, *kps2 = a.kps + (size_t)f2 * cap;
    const amos_sim3_point *pts1 = a.points + (size_t)f1 * cap, *pts2 = a.points + (size_t)f2 * cap;
    const amos_sim3_camera &c1 = a.cameras[f1], &c2 = a.cameras[f2];
    const int *in = a.matchIn + row;
    int *out = a.matchOut + row;
    so::Corr *corrs = a.corrs + row;
    uint8_t *level = a.level + row;
    if (out != in)
        for (int i = t; i < cap; i += kT) out[i] = in[i];

    // ---- the correspondences, in ascending order of keyframe 1's feature
    int bad = 0;
    const int n = block_compact<kT>(n1, sWave, [&](int i) {
        const int j = in[i];
        if (j < 0 || j >= n2) return false;
        if ((pts1[i].flags & AMOS_SIM3_POINT_SKIP) || (pts2[j].flags & AMOS_SIM3_POINT_SKIP)) return false;
        const int o1 = kps1[i].octave, o2 = kps2[j].octave;
        if (o1 < 0 || o1 >= a.nLevels || o2 < 0 || o2 >= a.nLevels) { bad |= so::kStatusOctave; return false; }
        return true;
    }, [&](int i, int c) {
        if (c < 0) return;
        const int j = in[i];
        const amos_keypoint k1 = kps1[i], k2 = kps2[j];
        so::Corr e;
        sim3::to_camera(c1.Rcw, c1.tcw, pts1[i].pos, e.P1);
        sim3::to_camera(c2.Rcw, c2.tcw, pts2[j].pos, e.P2);
        e.o1[0] = k1.x; e.o1[1] = k1.y; e.o2[0] = k2.x; e.o2[1] = k2.y;
        e.w1 = a.invSigma2[k1.octave]; e.w2 = a.invSigma2[k2.octave];
        e.feat = i; e.j = j;
        corrs[c] = e;
        level[c] = 0;
    });
    const int status = block_sum<kT>(bad, sWave) ? so::kStatusOctave : 0;
    if (t == 0) {
        so::pose_from_floats(R12, t12, s12, pr.fix_scale, sInit);
        so::out_begin(sOut, sInit, R12, t12, s12, c2.Rcw, c2.tcw, n, status);
    }
    if (n == 0) {  // (uniform) nothing to optimise: return 0, the Sim3 untouched
        if (t == 0) a.result[p] = *reinterpret_cast<const amos_sim3_opt_result *>(&sOut);
        return;
    }
    if (t == 0) {
        so::Cams &cams = sCams;
        cams.k1[0] = (double)c1.fx; cams.k1[1] = (double)c1.fy; cams.k1[2] = (double)c1.cx; cams.k1[3] = (double)c1.cy;
        cams.k2[0] = (double)c2.fx; cams.k2[1] = (double)c2.fy; cams.k2[2] = (double)c2.cx; cams.k2[3] = (double)c2.cy;
    }
    if (t < 2 * so::kDim) so::perturbation(t, pr.fix_scale, sUpd[t]);
    const so::Cams &cams = sCams;
    const float th2 = pr.th2;
    const double delta = so::huber_delta(th2);

    int nActive = n, nBadFirst = 0;
    for (int round = 0; round < 2; round++) {
        if (t == 0)
            lm_round_begin(lm, sInit, round == 0 ? so::kFirstIterations : (nBadFirst > 0 ? so::kMoreIterationsBad : so::kMoreIterationsClean));
        __syncthreads();  // the correspondences, sInit and lm are visible
        int act = po::kActIterate;
        while (act != po::kActRoundEnd) {
            // the 14 estimates of the numeric Jacobian, then computeActiveErrors + buildSystem at lm.cur
            if (t < 2 * so::kDim) so::update_apply(sUpd[t], lm.cur, sPert[t]);
            __syncthreads();
            // the partials live in LDS, one column per thread: 36 doubles in registers beside the Jacobian and the constants of the
            // single-lane code do not fit without scratch
            double *acc = &sAcc[0][t];
#pragma unroll
            for (int k = 0; k < so::kSums; k++) acc[k * kT] = 0.0;
            for (int c = t; c < n; c += kT)
                if (level[c] == 0) so::corr_accumulate<kT>(lm.cur, sPert, cams, corrs[c], delta, acc);
#pragma unroll
            for (int k = 0; k < so::kSums; k++) {
                const double v = s3o_wave_fold(acc[k * kT]);
                if (lane == 0) sPart[wv][k] = v;
            }
            __syncthreads();
            if (t < so::kSums) sSums[t] = so::add(so::add(sPart[0][t], sPart[1][t]), so::add(sPart[2][t], sPart[3][t]));
            __syncthreads();
            if (t == 0) lm_iteration_begin(lm, sSums);
            __syncthreads();
            do {  // the trials: the robust chi2 at lm.trial
                double c2sum = 0.0;
                for (int c = t; c < n; c += kT)
                    if (level[c] == 0) c2sum = so::corr_robust_chi2(lm.trial, cams, corrs[c], delta, c2sum);
                c2sum = s3o_wave_fold(c2sum);
                if (lane == 0) sPart[wv][0] = c2sum;
                __syncthreads();
                if (t == 0) sAct = lm_trial_done(lm, so::add(so::add(sPart[0][0], sPart[1][0]), so::add(sPart[2][0], sPart[3][0])));
                __syncthreads();
                act = sAct;  // the same value in every thread: the loops' barriers stay uniform
            } while (act == po::kActTrial);
        }
        // classification with each edge's error at the last evaluated estimate; a bad correspondence clears its entry and leaves
        int mine = 0;
        for (int c = t; c < n; c += kT) {
            if (level[c] != 0) continue;
            const so::Corr e = corrs[c];
            if (so::corr_is_bad(lm.lastEval, cams, e, th2)) {
                level[c] = 1;
                out[e.feat] = -1;
                mine++;
            }
        }
        const int nBad = block_sum<kT>(mine, sWave);
        if (t == 0) {
            so::out_round(sOut, round, lm);
            if (round == 0) {
                sOut.n_bad_first = nBad;
                sInit = lm.cur;  // the vertex keeps its estimate into the second optimisation
            } else {
                so::out_final(sOut, lm.cur, c2.Rcw, c2.tcw, nActive - nBad);
            }
        }
        if (round == 0) {
            nBadFirst = nBad;
            nActive = n - nBad;
            if (nActive < so::kMinCorrespondences) break;  // (uniform) return 0: the record keeps the input Sim3
        }
    }
    if (t == 0) a.result[p] = *reinterpret_cast<const amos_sim3_opt_result *>(&sOut);
}

}  // namespace amos

using namespace amos;

static bool s3o_camera_ok(const char *name, const amos_sim3_camera &c, int k)
{
    bool ok = std::isfinite(c.fx) && std::isfinite(c.fy) && std::isfinite(c.cx) && std::isfinite(c.cy);
    for (int i = 0; i < 9; i++) ok = ok && std::isfinite(c.Rcw[i]);
    for (int i = 0; i < 3; i++) ok = ok && std::isfinite(c.tcw[i]);
    if (!ok) set_error("%s: camera %d is not finite", name, k);
    return ok;
}

static bool s3o_pair_ok(const char *name, const amos_sim3_opt_pair &p, bool hostSim3, int k)
{
    if ((p.fix_scale != 0 && p.fix_scale != 1) || (p.enabled != 0 && p.enabled != 1)) {
        set_error("%s: pair %d: fix_scale or enabled is neither 0 nor 1", name, k);
        return false;
    }
    if (!p.enabled) return true;
    if (!(std::isfinite(p.th2) && p.th2 > 0.f)) { set_error("%s: pair %d: th2 is not finite or <= 0", name, k); return false; }
    if (!hostSim3) return true;
    bool ok = std::isfinite(p.s12) && p.s12 > 0.f;
    for (int i = 0; i < 9; i++) ok = ok && std::isfinite(p.R12[i]);
    for (int i = 0; i < 3; i++) ok = ok && std::isfinite(p.t12[i]);
    if (!ok) set_error("%s: pair %d: the Sim3 is not finite or has s12 <= 0", name, k);
    return ok;
}

extern "C" {

int amos_match_sim3_optimize_batch_device(amos_match *m, const amos_sim3_optimize *s)
{
    static const char *name = "amos_match_sim3_optimize_batch_device";
    if (!m || !s || !s->d_kps || !s->d_counts || !s->d_points || !s->cameras || !s->d_pairs_1 || !s->d_pairs_2 || !s->inv_level_sigma2 || !s->pairs ||
        !s->d_match12 || !s->d_match_out || !s->d_result || s->n_pairs < 1 || s->n_frames < 1 || s->capacity < 1 || s->capacity > 65536 ||
        s->n_levels < 1 || s->n_levels > AMOS_MAX_LEVELS) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    for (int k = 0; k < s->n_frames; k++)
        if (!s3o_camera_ok(name, s->cameras[k], k)) return AMOS_ERR_INVALID;
    for (int k = 0; k < s->n_pairs; k++)
        if (!s3o_pair_ok(name, s->pairs[k], s->d_sim3 == nullptr, k)) return AMOS_ERR_INVALID;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    // the call's workspace: the pair records, the cameras, the correspondences and their levels
    const size_t np = (size_t)s->n_pairs, slots = np * (size_t)s->capacity;
    const size_t bytesPairs = align64(sizeof(amos_sim3_opt_pair) * np), bytesCams = align64(sizeof(amos_sim3_camera) * (size_t)s->n_frames),
                 bytesCorrs = align64(sizeof(so::Corr) * slots);
    int rc = grow(&m->dLocal, &m->capLocal, bytesPairs + bytesCams + bytesCorrs + align64(slots));
    if (rc != AMOS_OK) return rc;
    std::vector<uint8_t> host(bytesPairs + bytesCams, 0);
    std::memcpy(host.data(), s->pairs, sizeof(amos_sim3_opt_pair) * np);
    std::memcpy(host.data() + bytesPairs, s->cameras, sizeof(amos_sim3_camera) * (size_t)s->n_frames);
    rc = upload_frames(m, host.data(), host.size());
    if (rc != AMOS_OK) return rc;
    S3OptArgs a;
    a.kps = s->d_kps; a.counts = s->d_counts; a.points = s->d_points;
    a.pairs = (const amos_sim3_opt_pair *)m->dLocal; a.cameras = (const amos_sim3_camera *)(m->dLocal + bytesPairs);
    a.sim3 = s->d_sim3; a.pairs1 = s->d_pairs_1; a.pairs2 = s->d_pairs_2;
    a.matchIn = s->d_match12; a.matchOut = s->d_match_out; a.result = s->d_result;
    a.corrs = (so::Corr *)(m->dLocal + bytesPairs + bytesCams); a.level = m->dLocal + bytesPairs + bytesCams + bytesCorrs;
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.invSigma2[l] = l < s->n_levels ? s->inv_level_sigma2[l] : 0.f;
    a.capacity = s->capacity; a.nLevels = s->n_levels; a.nFrames = s->n_frames;
    hipLaunchKernelGGL(k_sim3_optimize, dim3(s->n_pairs), dim3(so::kThreads), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_sim3_optimize(amos_match *m, const amos_keypoint *kps1, const amos_sim3_point *points1, int n1, const amos_keypoint *kps2,
                             const amos_sim3_point *points2, int n2, const amos_sim3_camera *cameras, const int32_t *match12,
                             const float *inv_level_sigma2, int n_levels, const amos_sim3_opt_pair *pair, int32_t *match_out,
                             amos_sim3_opt_result *result)
{
    static const char *name = "amos_match_sim3_optimize";
    if (!m || !cameras || !inv_level_sigma2 || !pair || !result || n1 < 0 || n1 > 65536 || n2 < 0 || n2 > 65536 ||
        (n1 > 0 && (!kps1 || !points1 || !match12 || !match_out)) || (n2 > 0 && (!kps2 || !points2)) || n_levels < 1 || n_levels > AMOS_MAX_LEVELS) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    if (!s3o_camera_ok(name, cameras[0], 0) || !s3o_camera_ok(name, cameras[1], 1) || !s3o_pair_ok(name, *pair, true, 0)) return AMOS_ERR_INVALID;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t cap = (size_t)std::max(std::max(n1, n2), 1);
    const size_t bytesKps = sizeof(amos_keypoint) * cap, bytesPts = sizeof(amos_sim3_point) * cap, bytesMatch = sizeof(int32_t) * cap;
    const size_t oMatch = align64(sizeof(amos_sim3_opt_result)), oEnd = oMatch + align64(bytesMatch);
    int rc = stage_begin(m, 2 * (bytesKps + bytesPts) + bytesMatch + 64 * 10 + oEnd);
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, oEnd);
    if (rc != AMOS_OK) return rc;
    const int32_t counts[2] = {n1, n2}, slot1 = 0, slot2 = 1;
    amos_sim3_optimize s;
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
    s.cameras = cameras; s.inv_level_sigma2 = inv_level_sigma2; s.pairs = pair; s.d_sim3 = nullptr;
    uint8_t *out = (uint8_t *)m->dOut;
    s.d_result = (amos_sim3_opt_result *)out; s.d_match_out = (int32_t *)(out + oMatch);
    s.n_frames = 2; s.n_pairs = 1; s.capacity = (int32_t)cap; s.n_levels = n_levels;
    if ((rc = stage_flush(m)) != AMOS_OK || (rc = amos_match_sim3_optimize_batch_device(m, &s)) != AMOS_OK) return rc;
    uint8_t *h = m->hStage + stage_take(m, oEnd);
    AMOS_HIP_CHECK(hipMemcpyAsync(h, out, oEnd, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    std::memcpy(result, h, sizeof(amos_sim3_opt_result));
    if (n1 && !result->skipped && result->code == 0) std::memcpy(match_out, h + oMatch, sizeof(int32_t) * (size_t)n1);
    return AMOS_OK;
}

}  // extern "C"
