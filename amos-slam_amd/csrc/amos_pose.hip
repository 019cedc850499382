// amos_pose.hip -- Optimizer::PoseOptimization (Optimizer.cc:363-605) for a batch of resident frames, behind the searches that fill
// d_match (amos_motion.hip, amos_bow_search.hip, amos_local.hip): ONE launch, k_pose_optimize, one work-group of po::kThreads per frame.
// The prologue compacts the matched features into the frame's edge list (ascending feature index); the four rounds, their Levenberg
// iterations and trials all run inside the kernel.  Every thread sums its edges t, t + kThreads, ...; the partials are folded in the fixed
// order of po::tree_sum (amos_pose_core.h) by shuffles and one LDS exchange; thread 0 owns the Levenberg state (po::Lm, in LDS), solves the
// 6 x 6 system and leaves the next pose in LDS for all.  Every loop decision is read from LDS by all threads, so the barriers stay uniform.
// No atomics, nothing to zero between calls.  The arithmetic is defined in amos_pose_core.h; include/amos_frontend.h, "pose optimisation".
#include "amos_block.h"
#include "amos_match_core.h"
#include "amos_pose_core.h"
#include "amos_projection_search.h"  // align64, upload_frames

#include <vector>

namespace amos {

static_assert(sizeof(amos_pose_camera) == 68, "amos_pose_camera is 68 bytes");
static_assert(sizeof(amos_pose_result) == 272 && sizeof(po::Out) == 272, "amos_pose_result is po::Out: 272 bytes");
static_assert(sizeof(po::Edge) == 32, "po::Edge is 32 bytes");

struct PoseFrame {
    amos_pose_camera cam;
    int off0, off1;  // the frame's points
};

struct PoseArgs {
    const amos_keypoint *kps;  // [frames][capacity]
    const float *uRight;       // [frames][capacity] or null
    const int *counts;
    int *match;                // [frames][capacity]
    const uint8_t *points;     // records of pointStride bytes that begin with float pos[3]
    const PoseFrame *frames;
    uint8_t *outlier;          // [frames][capacity]
    amos_pose_result *result;
    po::Edge *edges;           // scratch [frames][capacity]
    uint8_t *level;            // scratch [frames][capacity]: 1 = the edge is an outlier (g2o's level 1)
    float invSigma2[AMOS_MAX_LEVELS];
    int pointStride, flagsOffset, hasObsBit;
    int capacity, nLevels, clearOutliers;
};

// the fold of po::tree_sum inside one wave: lane i < s takes p[i] + p[i + s] for s = 32 .. 1 (addition commutes, so the xor partner serves)
__device__ __forceinline__ double wave_fold(double v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = po::add(v, __shfl_xor(v, s, 64));
    return v;
}

// R | t of a pose in LDS -> registers (the edges read nothing else)
__device__ __forceinline__ void load_Rt(const po::Pose &src, po::Pose &dst)
{
#pragma unroll
    for (int i = 0; i < 9; i++) dst.R[i] = src.R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) dst.t[i] = src.t[i];
}

// grid = frames, block = po::kThreads
__global__ __launch_bounds__(po::kThreads) void k_pose_optimize(const PoseArgs a)
{
    constexpr int kT = po::kThreads, kWaves = kT / 64;
    __shared__ po::Lm lm;
    __shared__ po::Pose sInit;
    __shared__ po::Out sOut;
    __shared__ double sPart[kWaves][po::kSums];
    __shared__ double sSums[po::kSums];
    __shared__ int sWave[kWaves];
    __shared__ int sAct;
    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const PoseFrame &fr = a.frames[f];
    const int cap = a.capacity, cnt = min(max(a.counts[f], 0), cap), nPts = fr.off1 - fr.off0;
    const size_t o = (size_t)f * cap;
    const amos_keypoint *kps = a.kps + o;
    const float *ur = a.uRight ? a.uRight + o : nullptr;
    int *match = a.match + o;
    uint8_t *outlier = a.outlier + o, *level = a.level + o;
    po::Edge *edges = a.edges + o;
    const uint8_t *points = a.points + (size_t)fr.off0 * a.pointStride;

    // ---- the edge list: matched features in ascending order
    int bad = 0;
    const int nEdges = block_compact<kT>(cnt, sWave, [&](int i) {
        const int mi = match[i];
        if (mi < 0) return false;
        const int oct = kps[i].octave;
        if (oct < 0 || oct >= a.nLevels) { bad |= po::kStatusOctave; return false; }
        if (mi >= nPts) { bad |= po::kStatusMatchIndex; return false; }
        return true;
    }, [&](int i, int c) {
        if (c < 0) return;
        const amos_keypoint k = kps[i];
        const float *p = reinterpret_cast<const float *>(points + (size_t)match[i] * a.pointStride);
        po::Edge e;
        e.u = k.x; e.v = k.y; e.ur = ur ? ur[i] : -1.0f;
        e.X = p[0]; e.Y = p[1]; e.Z = p[2];
        e.w = a.invSigma2[k.octave];
        e.feat = i;
        edges[c] = e;
        level[c] = 0;
    });
    const int badOct = block_sum<kT>(bad & po::kStatusOctave, sWave), badIdx = block_sum<kT>(bad & po::kStatusMatchIndex, sWave);
    const int status = (badOct ? po::kStatusOctave : 0) | (badIdx ? po::kStatusMatchIndex : 0);
    if (t == 0) po::out_begin(sOut, fr.cam.Rcw, fr.cam.tcw, nEdges, status);
    if (nEdges < 3) {  // (uniform) return 0, pose and flags untouched
        if (t == 0) a.result[f] = *reinterpret_cast<const amos_pose_result *>(&sOut);
        return;
    }
    if (t == 0) po::pose_from_floats(fr.cam.Rcw, fr.cam.tcw, sInit);
    const po::Cam cam{(double)fr.cam.fx, (double)fr.cam.fy, (double)fr.cam.cx, (double)fr.cam.cy, (double)fr.cam.mbf};
    __syncthreads();  // the edge list and sInit are visible

    int nBad = 0;
    for (int round = 0; round < po::kRounds; round++) {
        const bool huber = round < 3;
        if (t == 0) po::lm_round_begin(lm, sInit);
        int mine = 0;
        for (int e = t; e < nEdges; e += kT) mine += level[e] == 0;
        const int nActive = block_sum<kT>(mine, sWave);  // (its barriers publish lm)
        int act = nActive > 0 ? po::kActIterate : po::kActRoundEnd;
        while (act != po::kActRoundEnd) {
            // computeActiveErrors + buildSystem at lm.cur
            po::Pose T;
            load_Rt(lm.cur, T);
            double acc[po::kSums];
#pragma unroll
            for (int k = 0; k < po::kSums; k++) acc[k] = 0.0;
            for (int e = t; e < nEdges; e += kT)
                if (level[e] == 0) po::edge_accumulate(T, cam, edges[e], huber, acc);
#pragma unroll
            for (int k = 0; k < po::kSums; k++) {
                const double v = wave_fold(acc[k]);
                if (lane == 0) sPart[wv][k] = v;
            }
            __syncthreads();
            if (t < po::kSums) sSums[t] = po::add(po::add(sPart[0][t], sPart[1][t]), po::add(sPart[2][t], sPart[3][t]));
            __syncthreads();
            if (t == 0) po::lm_iteration_begin(lm, sSums);
            __syncthreads();
            do {  // the trials: the robust chi2 at lm.trial
                load_Rt(lm.trial, T);
                double c = 0.0;
                for (int e = t; e < nEdges; e += kT)
                    if (level[e] == 0) c = po::add(c, po::edge_robust_chi2(T, cam, edges[e], huber));
                c = wave_fold(c);
                if (lane == 0) sPart[wv][0] = c;
                __syncthreads();
                if (t == 0) sAct = po::lm_trial_done(lm, po::add(po::add(sPart[0][0], sPart[1][0]), po::add(sPart[2][0], sPart[3][0])));
                __syncthreads();
                act = sAct;  // the same value in every thread: the loops' barriers stay uniform
            } while (act == po::kActTrial);
        }
        // classification: an outlier edge is computed again at the round's pose, an inlier keeps the error of the last evaluation
        po::Pose A, B;
        load_Rt(lm.cur, A);
        load_Rt(lm.lastEval, B);
        mine = 0;
        for (int e = t; e < nEdges; e += kT) {
            const po::Edge ed = edges[e];
            double pc[3], err[3];
            const double chi2 = level[e] ? po::edge_error(A, cam, ed, pc, err) : po::edge_error(B, cam, ed, pc, err);
            const int out = po::edge_is_outlier(chi2, !(ed.ur < 0.0f)) ? 1 : 0;
            level[e] = (uint8_t)out;
            mine += out;
        }
        nBad = block_sum<kT>(mine, sWave);
        if (t == 0) po::out_round(sOut, round, lm);
        __syncthreads();  // lm is read before the next round resets it
        if (nEdges < 10) break;
    }

    // ---- mvbOutlier, and the discard loop of Tracking.cc:1770-1791 when asked for
    int mine = 0;
    for (int e = t; e < nEdges; e += kT) {
        const int i = edges[e].feat;
        if (level[e] == 0) {
            outlier[i] = 0;
            if (a.flagsOffset < 0) mine++;
            else mine += (*reinterpret_cast<const int *>(points + (size_t)match[i] * a.pointStride + a.flagsOffset) & a.hasObsBit) != 0;
        } else if (a.clearOutliers) {
            match[i] = -1;
            outlier[i] = 0;
        } else {
            outlier[i] = 1;
        }
    }
    const int nObs = block_sum<kT>(mine, sWave);
    if (t == 0) {
        po::pose_store(sOut.Rt, sOut.Tcw, sOut.Ow);
        sOut.n_inliers = nEdges - nBad;
        sOut.n_inliers_with_obs = nObs;
        a.result[f] = *reinterpret_cast<const amos_pose_result *>(&sOut);
    }
}

}  // namespace amos

using namespace amos;

extern "C" {

int amos_match_pose_optimization_batch_device(amos_match *m, const amos_pose_optimization *s)
{
    const char *name = "amos_match_pose_optimization_batch_device";
    if (!m || !s || !s->d_kps || !s->d_counts || !s->d_match || !s->d_points || !s->point_off || !s->cameras || !s->inv_level_sigma2 ||
        !s->d_outlier || !s->d_result || s->n_frames < 1 || s->capacity < 1 || s->capacity > 65536 || s->n_levels < 1 ||
        s->n_levels > AMOS_MAX_LEVELS || s->point_stride < 12 || s->point_stride % 4 != 0 ||
        !(s->flags_offset == -1 || (s->flags_offset >= 12 && s->flags_offset % 4 == 0 && s->flags_offset + 4 <= s->point_stride)) ||
        (s->clear_outliers != 0 && s->clear_outliers != 1)) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    if (s->point_off[0] < 0) { set_error("%s: point_off[0] < 0", name); return AMOS_ERR_INVALID; }
    for (int f = 0; f < s->n_frames; f++)
        if (s->point_off[f + 1] < s->point_off[f]) { set_error("%s: point_off descends at %d", name, f); return AMOS_ERR_INVALID; }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t slots = (size_t)s->n_frames * (size_t)s->capacity;
    const size_t bytesFrames = align64(sizeof(PoseFrame) * (size_t)s->n_frames), bytesEdges = align64(sizeof(po::Edge) * slots);
    int rc = grow(&m->dLocal, &m->capLocal, bytesFrames + bytesEdges + align64(slots));
    if (rc != AMOS_OK) return rc;
    std::vector<PoseFrame> frames((size_t)s->n_frames);
    for (int f = 0; f < s->n_frames; f++) frames[f] = PoseFrame{s->cameras[f], s->point_off[f], s->point_off[f + 1]};
    rc = upload_frames(m, frames.data(), sizeof(PoseFrame) * frames.size());
    if (rc != AMOS_OK) return rc;
    PoseArgs a;
    a.kps = s->d_kps; a.uRight = s->d_u_right; a.counts = s->d_counts; a.match = s->d_match;
    a.points = (const uint8_t *)s->d_points; a.frames = (const PoseFrame *)m->dLocal;
    a.outlier = s->d_outlier; a.result = s->d_result;
    a.edges = (po::Edge *)(m->dLocal + bytesFrames); a.level = m->dLocal + bytesFrames + bytesEdges;
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.invSigma2[l] = l < s->n_levels ? s->inv_level_sigma2[l] : 0.f;
    a.pointStride = s->point_stride; a.flagsOffset = s->flags_offset; a.hasObsBit = s->has_obs_bit;
    a.capacity = s->capacity; a.nLevels = s->n_levels; a.clearOutliers = s->clear_outliers;
    hipLaunchKernelGGL(k_pose_optimize, dim3(s->n_frames), dim3(po::kThreads), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_pose_optimization(amos_match *m, const amos_keypoint *kps_un, const float *u_right, int n, int32_t *match, const float *points_xyz,
                                 const uint8_t *has_obs, int n_points, const amos_pose_camera *camera, const float *inv_level_sigma2, int n_levels,
                                 int clear_outliers, uint8_t *outlier, amos_pose_result *result)
{
    if (!m || !camera || !inv_level_sigma2 || !result || n < 0 || n > 65536 || n_points < 0 || (n > 0 && (!kps_un || !match || !outlier)) ||
        (n_points > 0 && !points_xyz) || n_levels < 1 || n_levels > AMOS_MAX_LEVELS || (clear_outliers != 0 && clear_outliers != 1)) {
        set_error("amos_match_pose_optimization: invalid argument");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    struct Point { float pos[3]; int32_t flags; };
    const size_t cap = (size_t)std::max(n, 1), np1 = (size_t)std::max(n_points, 1);
    const size_t bytesMatch = sizeof(int32_t) * cap, bytesOut = align64(bytesMatch) + align64(cap) + align64(sizeof(amos_pose_result));
    int rc = stage_begin(m, cap * (sizeof(amos_keypoint) + 4 + 4 + 1) + np1 * sizeof(Point) + 64 * 8 + bytesOut);
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, sizeof(amos_pose_result));
    if (rc != AMOS_OK) return rc;
    const std::vector<uint8_t> zeros(cap * sizeof(amos_keypoint), 0);  // a frame without features still hands valid arrays down
    std::vector<Point> pts(np1, Point{{0.f, 0.f, 0.f}, 0});
    for (int p = 0; p < n_points; p++) pts[p] = Point{{points_xyz[3 * p], points_xyz[3 * p + 1], points_xyz[3 * p + 2]}, (!has_obs || has_obs[p]) ? 1 : 0};
    const int32_t count = n, off[2] = {0, n_points};
    amos_pose_optimization s;
    s.d_kps = stage_input<amos_keypoint>(m, n ? (const void *)kps_un : zeros.data(), sizeof(amos_keypoint) * cap);
    s.d_u_right = u_right && n ? stage_input<float>(m, u_right, sizeof(float) * cap) : nullptr;
    s.d_counts = stage_input<int32_t>(m, &count, sizeof(count));
    s.d_match = stage_input<int32_t>(m, n ? (const void *)match : zeros.data(), bytesMatch);
    s.d_points = stage_input<Point>(m, pts.data(), sizeof(Point) * np1);
    s.point_stride = (int32_t)sizeof(Point); s.flags_offset = 12; s.has_obs_bit = 1;
    s.point_off = off; s.cameras = camera; s.inv_level_sigma2 = inv_level_sigma2;
    s.d_outlier = stage_input<uint8_t>(m, n ? outlier : zeros.data(), cap);
    s.d_result = (amos_pose_result *)m->dOut;
    s.n_frames = 1; s.capacity = (int32_t)cap; s.n_levels = n_levels; s.clear_outliers = clear_outliers;
    if ((rc = stage_flush(m)) != AMOS_OK || (rc = amos_match_pose_optimization_batch_device(m, &s)) != AMOS_OK) return rc;
    uint8_t *hMatch = m->hStage + stage_take(m, bytesMatch), *hOutlier = m->hStage + stage_take(m, cap), *hResult = m->hStage + stage_take(m, sizeof(amos_pose_result));
    AMOS_HIP_CHECK(hipMemcpyAsync(hMatch, s.d_match, bytesMatch, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipMemcpyAsync(hOutlier, s.d_outlier, cap, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipMemcpyAsync(hResult, s.d_result, sizeof(amos_pose_result), hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (n) {
        std::memcpy(match, hMatch, sizeof(int32_t) * (size_t)n);
        std::memcpy(outlier, hOutlier, (size_t)n);
    }
    std::memcpy(result, hResult, sizeof(amos_pose_result));
    return AMOS_OK;
}

}  // extern "C"
