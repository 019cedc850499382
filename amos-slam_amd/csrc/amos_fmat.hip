// amos_fmat.hip -- cv::findFundamentalMat(p1, p2, FM_RANSAC, 0.1, 0.99) of Tracking::GetSceneFlowObj (src/Tracking.cc:927, 945) on the
// device: the whole RANSAC (sampler, 7-point solver, scoring, best-model rule, iteration-count update) for n >= 15 correspondences.
// The arithmetic is amos_fmat_core.h (restated; parity with OpenCV unpinned); the round's draw, scorer and sequential
// replay are amos_ransac.h (shared with amos_pnp.hip), the compaction amos_block.h.
//   k_fmat_ransac   ONE WORK-GROUP PER PROBLEM (a batch of problems is one launch).  The selected points go to LDS (16 B each), then
//                   rounds of up to 64 iterations: wave 0 runs the serial RNG (every lane the same state, collinearity pairs over the
//                   lanes) and draws the next subsets; one lane per subset solves run7Point; all waves score the up to 192 models over all
//                   points (counts by wave reduction, no atomics); one lane replays the sequential loop in iteration order (best model,
//                   niters).  The RNG consumption depends only on the points, never on the scores, so drawing ahead changes nothing.
//   k_fmat_keep     Tracking.cc:928-944: keep = state != 0 && dd <= 0.5 under the first F (epipolar_distance, amos_scene_flow.h)
#include "amos_common.h"
#include "amos_fmat_core.h"
#include "amos_ransac.h"
#include "amos_scene_flow.h"

namespace amos {

constexpr int kFmatMaxPoints = 4096;
constexpr int kFmatThreads = 512, kFmatWaves = kFmatThreads / 64;
constexpr int kFmatRound = 64;

struct FmatArgs {
    const float2 *p1, *p2;
    const int *offsets, *counts;
    const uint8_t *select;
    int maxPoints, maxIters;
    float thresh2;
    double confidence;
    double *F;
    int *status;
    uint8_t *mask;
};

__global__ __launch_bounds__(kFmatThreads) void k_fmat_ransac(const FmatArgs a)
{
    __shared__ float4 sPts[kFmatMaxPoints];                 // (x1, y1, x2, y2) of the selected points
    __shared__ double sModel[kFmatRound * 3][9];
    __shared__ int sCount[kFmatRound * 3], sNModels[kFmatRound], sSub[kFmatRound][7];
    __shared__ double sBest[9];
    __shared__ int sWave[kFmatWaves];
    __shared__ ransac::State sR;
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int off = a.offsets ? a.offsets[p] : p * a.maxPoints, cnt = a.counts[p];
    double *Fout = a.F + (size_t)p * 9;
    int *st = a.status + (size_t)p * 4;
    uint8_t *mask = a.mask ? a.mask + off : nullptr;
    if (cnt < 0 || cnt > a.maxPoints) {  // out of range: nothing is read, no mask written
        ransac::no_model<kFmatThreads, 9, 4>(Fout, st, -3, 0, 0, nullptr, 0);
        return;
    }
    auto selected = [&](int i) { return !a.select || a.select[off + i] != 0; };
    const int n = block_compact<kFmatThreads>(cnt, sWave, selected, [&](int i, int c) {
        if (c >= 0) sPts[c] = make_float4(a.p1[off + i].x, a.p1[off + i].y, a.p2[off + i].x, a.p2[off + i].y);
    });
    ransac::begin(sR, a.maxIters);
    if (n < 15) {  // n < 7: no model; 7 <= n < 15: OpenCV's LMeDS / 7-point branches (not built here)
        ransac::no_model<kFmatThreads, 9, 4>(Fout, st, n < 7 ? 0 : -1, 0, n, mask, cnt);
        return;
    }
    __syncthreads();
    auto error_of = [&](const double *F, int i) {
        const float4 P = sPts[i];
        return fm::point_error(F, P.x, P.y, P.z, P.w);
    };
    uint64_t rng = ~0ull;  // cv::RNG rng((uint64)-1), wave 0's lanes hold identical copies
    for (;;) {
        const int limit = min(kFmatRound, sR.niters - sR.iter);
        // ---- draw the subsets of iterations iter .. iter + limit - 1 (getSubset, maxAttempts 10000)
        if (wv == 0) {
            int drawn = 0, stop = 0;
            for (int slot = 0; slot < limit; slot++) {
                int idx[7];
                bool found = false, cap = false;
                for (int attempt = 0; attempt < fm::kMaxAttempts && !found && !cap; attempt++) {
                    cap = !ransac::draw_distinct<7>(rng, n, idx);
                    if (cap) break;
                    bool col = false;  // FMEstimatorCallback::checkSubset: lanes 0..14 set 1, 15..29 set 2
                    if (lane < 30) {
                        const int q = lane < 15 ? lane : lane - 15, j = FM_PAIR_J(q), k = FM_PAIR_K(q);
                        int ij = idx[0], ik = idx[0];
#pragma unroll
                        for (int u = 1; u < 6; u++) { ij = u == j ? idx[u] : ij; ik = u == k ? idx[u] : ik; }
                        const float4 Pj = sPts[ij], Pk = sPts[ik], Pi = sPts[idx[6]];
                        col = lane < 15 ? fm::collinear3(Pj.x, Pj.y, Pk.x, Pk.y, Pi.x, Pi.y) : fm::collinear3(Pj.z, Pj.w, Pk.z, Pk.w, Pi.z, Pi.w);
                    }
                    found = __ballot(col) == 0ull;
                }
                if (cap) { stop = 2; break; }
                if (!found) { stop = 1; break; }
                if (lane < 7) {
                    int v = idx[0];
#pragma unroll
                    for (int u = 1; u < 7; u++) v = u == lane ? idx[u] : v;
                    sSub[slot][lane] = v;
                }
                drawn++;
            }
            if (lane == 0) { sR.drawn = drawn; sR.stop = stop; }
        }
        __syncthreads();
        const int drawn = sR.drawn;
        // ---- run7Point, one lane per subset
        if (t < drawn) {
            float x0[7], y0[7], x1[7], y1[7];
#pragma unroll
            for (int i = 0; i < 7; i++) {
                const float4 P = sPts[sSub[t][i]];
                x0[i] = P.x; y0[i] = P.y; x1[i] = P.z; y1[i] = P.w;
            }
            double F[27];
            const int nm = fm::run7point(x0, y0, x1, y1, F);
            sNModels[t] = nm;
            for (int m = 0; m < nm; m++)
#pragma unroll
                for (int k = 0; k < 9; k++) sModel[3 * t + m][k] = F[9 * m + k];
        }
        __syncthreads();
        // ---- scoring: model m = 3 * slot + root
        ransac::score_models<kFmatThreads>(sModel, 3 * drawn, n, a.thresh2, sCount, [&](int m) { return m % 3 < sNModels[m / 3]; }, error_of);
        __syncthreads();
        if (t == 0) ransac::replay_round<9, 3, fm::kModelPoints>(sR, n, a.confidence, sModel, sNModels, sCount, sBest);
        __syncthreads();
        if (sR.stop == 3) break;
    }
    // ---- result, F, mask of the best model
    const int result = ransac::result_of(sR), maxGood = result == 1 ? sR.maxGood : 0;
    if (t < 9) Fout[t] = result == 1 ? sBest[t] : 0.0;
    if (t == 0) { st[0] = result; st[1] = maxGood; st[2] = sR.iter; st[3] = n; }
    if (mask) {
        double F[9];
#pragma unroll
        for (int k = 0; k < 9; k++) F[k] = sBest[k];
        block_compact<kFmatThreads>(cnt, sWave, selected, [&](int i, int c) { mask[i] = c >= 0 && result == 1 && error_of(F, c) <= a.thresh2 ? 1 : 0; });
    }
}

// keep[i] = state[i] != 0 && dd[i] <= 0.5 with dd of Tracking.cc:930-935 under F1; all 0 when F1 is no model
__global__ __launch_bounds__(256) void k_fmat_keep(const float2 *__restrict__ pre, const float2 *__restrict__ next, const uint8_t *__restrict__ state,
                                                  const int *__restrict__ dN, int maxPoints, const double *__restrict__ F, const int *__restrict__ status1,
                                                  uint8_t *__restrict__ keep)
{
    const int i = blockIdx.x * 256 + threadIdx.x, n = *dN;
    if (n < 0 || n > maxPoints || i >= n) return;
    uint8_t k = 0;
    if (status1[0] == 1 && state[i] != 0) {
        k = epipolar_distance(F, pre[i].x, pre[i].y, next[i].x, next[i].y) <= 0.5 ? 1 : 0;
    }
    keep[i] = k;
}

}  // namespace amos

using namespace amos;

struct amos_fmat : StreamHandle {
    int maxPoints = 0, maxProblems = 0;
    float2 *dP1 = nullptr, *dP2 = nullptr;
    int *dInt = nullptr;  // [0] zero offset, [1] count of the synchronous call, [2..5] its status
    double *dF = nullptr;
    uint8_t *dMask = nullptr;
};

static int fmat_launch(amos_fmat *h, int n_problems, const float *d_p1, const float *d_p2, const int *d_offsets, const int *d_counts, const uint8_t *d_select,
                       double threshold, double confidence, int max_iters, double *d_F, int *d_status, uint8_t *d_mask)
{
    FmatArgs a;
    a.p1 = (const float2 *)d_p1; a.p2 = (const float2 *)d_p2;
    a.offsets = d_offsets; a.counts = d_counts; a.select = d_select;
    a.maxPoints = h->maxPoints; a.maxIters = max_iters;
    a.thresh2 = (float)(threshold * threshold);  // findInliers: float t = (float)(thresh * thresh)
    a.confidence = confidence;
    a.F = d_F; a.status = d_status; a.mask = d_mask;
    hipLaunchKernelGGL(k_fmat_ransac, dim3(n_problems), dim3(kFmatThreads), 0, h->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

extern "C" {

int amos_fmat_create(int device, void *stream, int max_points, int max_problems, amos_fmat **out)
{
    if (!out || max_points < 1 || max_points > kFmatMaxPoints || max_problems < 1) {
        set_error("amos_fmat_create: invalid argument (1 <= max_points <= %d, max_problems >= 1)", kFmatMaxPoints);
        return AMOS_ERR_INVALID;
    }
    *out = nullptr;
    amos_fmat *h = new amos_fmat();
    h->maxPoints = max_points; h->maxProblems = max_problems;
    const int rc = h->open(device, stream);
    if (rc != AMOS_OK) { delete h; return rc; }
    hipError_t e = hipMalloc((void **)&h->dP1, sizeof(float2) * max_points);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dP2, sizeof(float2) * max_points);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dInt, sizeof(int) * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dF, sizeof(double) * 9);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dMask, max_points);
    if (e == hipSuccess) e = hipMemsetAsync(h->dInt, 0, sizeof(int) * 8, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { set_error("amos_fmat_create: %s", hipGetErrorString(e)); amos_fmat_destroy(h); return AMOS_ERR_DEVICE; }
    *out = h;
    return AMOS_OK;
}

void amos_fmat_destroy(amos_fmat *h)
{
    if (!h) return;
    h->close();
    for (void *q : {(void *)h->dP1, (void *)h->dP2, (void *)h->dInt, (void *)h->dF, (void *)h->dMask}) if (q) (void)hipFree(q);
    delete h;
}

void *amos_fmat_stream(amos_fmat *h) { return h ? (void *)h->stream : nullptr; }

int amos_fmat_ransac_device(amos_fmat *h, int n_problems, const float *d_p1_xy, const float *d_p2_xy, const int32_t *d_offsets, const int32_t *d_counts,
                            const uint8_t *d_select, double threshold, double confidence, int max_iters, double *d_F, int32_t *d_status, uint8_t *d_mask)
{
    if (!h || n_problems < 0 || n_problems > h->maxProblems || !d_p1_xy || !d_p2_xy || !d_counts || !d_F || !d_status ||
        !ransac_params_ok(threshold, confidence, max_iters)) {
        set_error("amos_fmat_ransac_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    if (n_problems == 0) return AMOS_OK;
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    return fmat_launch(h, n_problems, d_p1_xy, d_p2_xy, d_offsets, d_counts, d_select, threshold, confidence, max_iters, d_F, d_status, d_mask);
}

int amos_fmat_scene_flow_pair_device(amos_fmat *h, const float *d_pre_xy, const float *d_next_xy, const uint8_t *d_state, const int32_t *d_n, double *d_F1,
                                     double *d_F2, uint8_t *d_keep, int32_t *d_status)
{
    if (!h || !d_pre_xy || !d_next_xy || !d_state || !d_n || !d_F1 || !d_F2 || !d_keep || !d_status) {
        set_error("amos_fmat_scene_flow_pair_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    int rc = fmat_launch(h, 1, d_pre_xy, d_next_xy, h->dInt, d_n, d_state, 0.1, 0.99, 1000, d_F1, d_status, nullptr);
    if (rc != AMOS_OK) return rc;
    hipLaunchKernelGGL(k_fmat_keep, dim3((h->maxPoints + 255) / 256), dim3(256), 0, h->stream, (const float2 *)d_pre_xy, (const float2 *)d_next_xy, d_state, d_n,
                       h->maxPoints, d_F1, d_status, d_keep);
    AMOS_HIP_CHECK(hipGetLastError());
    return fmat_launch(h, 1, d_pre_xy, d_next_xy, h->dInt, d_n, d_keep, 0.1, 0.99, 1000, d_F2, d_status + 4, nullptr);
}

int amos_fmat_ransac(amos_fmat *h, int n, const float *p1_xy, const float *p2_xy, double threshold, double confidence, int max_iters, double *F,
                     uint8_t *mask, int32_t *status)
{
    if (!h || n < 0 || n > h->maxPoints || (n > 0 && (!p1_xy || !p2_xy)) || !F || !status || !ransac_params_ok(threshold, confidence, max_iters)) {
        set_error("amos_fmat_ransac: invalid argument (n <= max_points)");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    if (n > 0) {
        AMOS_HIP_CHECK(hipMemcpyAsync(h->dP1, p1_xy, sizeof(float2) * n, hipMemcpyHostToDevice, h->stream));
        AMOS_HIP_CHECK(hipMemcpyAsync(h->dP2, p2_xy, sizeof(float2) * n, hipMemcpyHostToDevice, h->stream));
    }
    AMOS_HIP_CHECK(hipMemcpyAsync(h->dInt + 1, &n, sizeof(int), hipMemcpyHostToDevice, h->stream));
    const int rc = fmat_launch(h, 1, (const float *)h->dP1, (const float *)h->dP2, h->dInt, h->dInt + 1, nullptr, threshold, confidence, max_iters, h->dF,
                               h->dInt + 2, h->dMask);
    if (rc != AMOS_OK) return rc;
    AMOS_HIP_CHECK(hipMemcpyAsync(F, h->dF, sizeof(double) * 9, hipMemcpyDeviceToHost, h->stream));
    AMOS_HIP_CHECK(hipMemcpyAsync(status, h->dInt + 2, sizeof(int) * 4, hipMemcpyDeviceToHost, h->stream));
    if (mask && n > 0) AMOS_HIP_CHECK(hipMemcpyAsync(mask, h->dMask, n, hipMemcpyDeviceToHost, h->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(h->stream));
    return AMOS_OK;
}

}  // extern "C"
