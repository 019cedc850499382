// amos_pnp.hip -- cv::solvePnPRansac(pre_3d, cur_2d, K, 0, rvec, tvec, false, 500, 0.4, 0.98, inliers, SOLVEPNP_P3P) of
// Tracking::GetSceneFlowObj (src/Tracking.cc:1006) on the device: the RANSAC over P3P samples and the EPnP refit on its inliers.
// The arithmetic is amos_pnp_core.h (restated; parity with OpenCV unpinned); the round's draw, scorer and sequential
// replay are amos_ransac.h (shared with amos_fmat.hip), the compaction amos_block.h.
//   k_pnp_ransac   ONE WORK-GROUP PER PROBLEM (a batch of problems is one launch).  The selected points go to LDS (20 B each), then
//                  rounds of up to 64 iterations: lane 0 runs the serial RNG and draws the subsets (PnPRansacCallback has no
//                  checkSubset, so every draw of 4 distinct indices is a subset); one lane per subset runs P3P; all waves score the up to
//                  64 models over all points (counts by wave reduction, no atomics); lane 0 replays the sequential loop in iteration order
//                  (best model, niters).  The RNG consumption depends only on the point count, so drawing ahead changes nothing.  Then
//                  the EPnP refit in the same launch (amos_pnp_block.h, shared with amos_reloc_pnp.hip): every sum over the inliers is
//                  owned by one lane and runs in inlier order; the per-inlier alphas and image points go through a global scratch row of
//                  the problem; the 12 x 12 Jacobi runs on sixteen lanes, the three beta sets on three, the other dense steps on one.
//   k_pnp_points   Tracking.cc:955-990: the N-point lists of the reference (pre_3d, cur_2d), (0, 0, 0) -> (0, 0) where a depth is missing
#include "amos_common.h"
#include "amos_pnp_block.h"
#include "amos_pnp_core.h"
#include "amos_ransac.h"
#include "amos_scene_flow.h"

namespace amos {

constexpr int kPnpMaxPoints = 4096;
constexpr int kPnpThreads = 512, kPnpWaves = kPnpThreads / 64;
constexpr int kPnpRound = 64;
constexpr int kPnpStatus = 5;
constexpr int kPnpScratch = pnp::kEpnpScratch;  // doubles per inlier: alphas[4], u, v

struct PnpArgs {
    const float *obj, *img;
    const int *offsets, *counts;
    const uint8_t *select;
    int maxPoints, maxIters;
    float thresh2;
    double confidence, fx, fy, cx, cy;
    double *Rt;
    int *status;
    uint8_t *mask;
    double *scratch;  // [problem][maxPoints][kPnpScratch]
};

__global__ __launch_bounds__(kPnpThreads) void k_pnp_ransac(const PnpArgs a)
{
    __shared__ float4 sP[kPnpMaxPoints];  // (X, Y, Z, u) of the selected points
    __shared__ float sV[kPnpMaxPoints];   // v
    __shared__ uint16_t sIdx[kPnpMaxPoints];  // compact indices of the refit's inliers
    __shared__ double sModel[kPnpRound][12];
    __shared__ int sOk[kPnpRound], sCount[kPnpRound], sSub[kPnpRound][4];
    __shared__ double sBest[12];
    __shared__ EpnpShared sE;
    __shared__ int sWave[kPnpWaves];
    __shared__ ransac::State sR;
    const int p = blockIdx.x, t = threadIdx.x;
    const int off = a.offsets ? a.offsets[p] : p * a.maxPoints, cnt = a.counts[p];
    double *Rout = a.Rt + (size_t)p * 12;
    int *st = a.status + (size_t)p * kPnpStatus;
    uint8_t *mask = a.mask ? a.mask + off : nullptr;
    if (cnt < 0 || cnt > a.maxPoints) {  // out of range: nothing is read, no mask written
        ransac::no_model<kPnpThreads, 12, kPnpStatus>(Rout, st, -3, 0, 0, nullptr, 0);
        return;
    }
    const float *obj = a.obj, *img = a.img;
    const uint8_t *select = a.select;
    auto selected = [&](int i) { return !select || select[off + i] != 0; };
    const int n = block_compact<kPnpThreads>(cnt, sWave, selected, [&](int i, int c) {
        if (c >= 0) {
            const size_t g = (size_t)(off + i);
            sP[c] = make_float4(obj[3 * g], obj[3 * g + 1], obj[3 * g + 2], img[2 * g]);
            sV[c] = img[2 * g + 1];
        }
    });
    const double fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy;
    if (n < pnp::kModelPoints) {  // OpenCV asserts: no model, too few points
        ransac::no_model<kPnpThreads, 12, kPnpStatus>(Rout, st, -1, 0, n, mask, cnt);
        return;
    }
    ransac::begin(sR, a.maxIters);
    if (n == pnp::kModelPoints) {  // solvePnPRansac's direct call: solvePnP(P3P) on the four points, all of them inliers
        if (t == 0) {
            float o[12], im[8];
            for (int i = 0; i < 4; i++) {
                o[3 * i] = sP[i].x; o[3 * i + 1] = sP[i].y; o[3 * i + 2] = sP[i].z;
                im[2 * i] = sP[i].w; im[2 * i + 1] = sV[i];
            }
            double M[12];
            const bool ok = pnp::p3p4(o, im, fx, fy, cx, cy, M);
            for (int k = 0; k < 12; k++) sBest[k] = ok ? M[k] : 0.0;
            sR.result = ok ? 1 : 0;
        }
        __syncthreads();
        const int ok = sR.result;
        if (t < 12) Rout[t] = sBest[t];
        if (t == 0) { st[0] = ok; st[1] = ok ? 4 : 0; st[2] = 0; st[3] = n; st[4] = 0; }
        if (mask) block_compact<kPnpThreads>(cnt, sWave, selected, [&](int i, int c) { mask[i] = c >= 0 && ok ? 1 : 0; });
        return;
    }
    __syncthreads();
    auto error_of = [&](const double *M, int i) {
        const float4 P = sP[i];
        return pnp::point_error(M, P.x, P.y, P.z, P.w, sV[i], fx, fy, cx, cy);
    };
    uint64_t rng = ~0ull;  // cv::RNG rng((uint64)-1), lane 0's copy
    for (;;) {
        const int limit = min(kPnpRound, sR.niters - sR.iter);
        // ---- draw the subsets of iterations iter .. iter + limit - 1 (getSubset: 4 distinct indices, no checkSubset)
        if (t == 0) {
            int drawn = 0, stop = 0;
            for (int slot = 0; slot < limit; slot++) {
                int idx[4];
                if (!ransac::draw_distinct<4>(rng, n, idx)) { stop = 2; break; }
                for (int i = 0; i < 4; i++) sSub[slot][i] = idx[i];
                drawn++;
            }
            sR.drawn = drawn; sR.stop = stop;
        }
        __syncthreads();
        const int drawn = sR.drawn;
        // ---- P3P, one lane per subset
        if (t < drawn) {
            float o[12], im[8];
            for (int i = 0; i < 4; i++) {
                const int c = sSub[t][i];
                const float4 P = sP[c];
                o[3 * i] = P.x; o[3 * i + 1] = P.y; o[3 * i + 2] = P.z;
                im[2 * i] = P.w; im[2 * i + 1] = sV[c];
            }
            double M[12];
            const bool ok = pnp::p3p4(o, im, fx, fy, cx, cy, M);
            sOk[t] = ok ? 1 : 0;
            for (int k = 0; k < 12; k++) sModel[t][k] = M[k];
        }
        __syncthreads();
        // ---- scoring: one model per slot, sOk its count
        ransac::score_models<kPnpThreads>(sModel, drawn, n, a.thresh2, sCount, [&](int m) { return sOk[m] != 0; }, error_of);
        __syncthreads();
        if (t == 0) ransac::replay_round<12, 1, pnp::kModelPoints>(sR, n, a.confidence, sModel, sOk, sCount, sBest);
        __syncthreads();
        if (sR.stop == 3) break;
    }
    const int result = ransac::result_of(sR);
    if (result != 1) {
        ransac::no_model<kPnpThreads, 12, kPnpStatus>(Rout, st, result, sR.iter, n, mask, cnt);
        return;
    }
    // ---- the RANSAC mask, the inlier list in order
    double B[12];
    for (int k = 0; k < 12; k++) B[k] = sBest[k];
    auto inlier = [&](int c) { return error_of(B, c) <= a.thresh2; };
    const int m = block_compact<kPnpThreads>(n, sWave, inlier, [&](int i, int c) { if (c >= 0) sIdx[c] = (uint16_t)i; });
    if (mask) block_compact<kPnpThreads>(cnt, sWave, selected, [&](int i, int c) { mask[i] = c >= 0 && inlier(c) ? 1 : 0; });
    // ---- EPnP on the m inliers (m = maxGood >= 4): amos_pnp_block.h, the image points through undistortPoints and back
    double *scr = a.scratch + (size_t)p * a.maxPoints * kPnpScratch;
    block_epnp<kPnpThreads, pnp::PixelRefit>(sE, m, [&](int j, double *pw) {
        const float4 P = sP[sIdx[j]];
        pw[0] = P.x; pw[1] = P.y; pw[2] = P.z;
    }, [&](int j, float &u, float &v) { u = sP[sIdx[j]].w; v = sV[sIdx[j]]; }, fx, fy, cx, cy, scr);
    if (t == 0) {
        const int N = epnp_pick(sE);
        bool ok = true;
        for (int k = 0; k < 12; k++) ok = ok && pnp::finite_(sE.Rt[N][k]);
        for (int k = 0; k < 12; k++) Rout[k] = ok ? sE.Rt[N][k] : sBest[k];
        st[0] = 1; st[1] = sR.maxGood; st[2] = sR.iter; st[3] = n; st[4] = ok ? 1 : -1;
    }
}

// the reference's N-point lists (Tracking.cc:955-990) for i < *d_n: pre_3d / cur_2d where z1 > 0 && z2 > 0, (0, 0, 0) / (0, 0) elsewhere
// (entries with state 0 are written too and not selected).  A pixel outside the depth map counts as a missing depth.
__global__ __launch_bounds__(256) void k_pnp_points(const float2 *__restrict__ pre, const float2 *__restrict__ next, const int *__restrict__ dN, int maxPoints,
                                                    const float *__restrict__ depthLast, size_t lastStride, const float *__restrict__ depthCur,
                                                    size_t curStride, int width, int height, const SceneFlowArgs sa, float *__restrict__ obj,
                                                    float *__restrict__ img)
{
    const int i = blockIdx.x * 256 + threadIdx.x, n = *dN;
    if (n < 0 || n > maxPoints || i >= n) return;
    const float2 P = pre[i], Q = next[i];
    float z1, z2;
    scene_flow_depths(depthLast, lastStride, depthCur, curStride, width, height, P, Q, z1, z2);
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, u = 0.f, v = 0.f;
    if (z1 > 0 && z2 > 0) {
        scene_flow_pre3d(sa, P.x, P.y, z1, o0, o1, o2);
        u = Q.x;
        v = Q.y;
    }
    obj[3 * i] = o0; obj[3 * i + 1] = o1; obj[3 * i + 2] = o2;
    img[2 * i] = u; img[2 * i + 1] = v;
}

}  // namespace amos

using namespace amos;

struct amos_pnp : StreamHandle {
    int maxPoints = 0, maxProblems = 0;
    float *dObj = nullptr, *dImg = nullptr;
    int *dInt = nullptr;  // [0] zero offset, [1] count of the synchronous call, [2..6] its status
    double *dRt = nullptr, *dScratch = nullptr;
    uint8_t *dMask = nullptr;
};

static int pnp_launch(amos_pnp *h, int n_problems, const float *d_obj, const float *d_img, const int *d_offsets, const int *d_counts, const uint8_t *d_select,
                      double fx, double fy, double cx, double cy, double reprojection_error, double confidence, int max_iters, double *d_Rt, int *d_status,
                      uint8_t *d_mask)
{
    PnpArgs a;
    a.obj = d_obj; a.img = d_img;
    a.offsets = d_offsets; a.counts = d_counts; a.select = d_select;
    a.maxPoints = h->maxPoints; a.maxIters = max_iters;
    a.thresh2 = (float)(reprojection_error * reprojection_error);  // findInliers: float t = (float)(thresh * thresh)
    a.confidence = confidence;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.Rt = d_Rt; a.status = d_status; a.mask = d_mask;
    a.scratch = h->dScratch;
    hipLaunchKernelGGL(k_pnp_ransac, dim3(n_problems), dim3(kPnpThreads), 0, h->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

extern "C" {

int amos_pnp_create(int device, void *stream, int max_points, int max_problems, amos_pnp **out)
{
    if (!out || max_points < 1 || max_points > kPnpMaxPoints || max_problems < 1 || max_problems > 65535) {
        set_error("amos_pnp_create: invalid argument (1 <= max_points <= %d, 1 <= max_problems <= 65535)", kPnpMaxPoints);
        return AMOS_ERR_INVALID;
    }
    *out = nullptr;
    amos_pnp *h = new amos_pnp();
    h->maxPoints = max_points; h->maxProblems = max_problems;
    const int rc = h->open(device, stream);
    if (rc != AMOS_OK) { delete h; return rc; }
    hipError_t e = hipMalloc((void **)&h->dObj, sizeof(float) * 3 * max_points);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dImg, sizeof(float) * 2 * max_points);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dInt, sizeof(int) * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dRt, sizeof(double) * 12);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dScratch, sizeof(double) * kPnpScratch * (size_t)max_points * max_problems);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dMask, max_points);
    if (e == hipSuccess) e = hipMemsetAsync(h->dInt, 0, sizeof(int) * 8, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { set_error("amos_pnp_create: %s", hipGetErrorString(e)); amos_pnp_destroy(h); return AMOS_ERR_DEVICE; }
    *out = h;
    return AMOS_OK;
}

void amos_pnp_destroy(amos_pnp *h)
{
    if (!h) return;
    h->close();
    for (void *q : {(void *)h->dObj, (void *)h->dImg, (void *)h->dInt, (void *)h->dRt, (void *)h->dScratch, (void *)h->dMask}) if (q) (void)hipFree(q);
    delete h;
}

void *amos_pnp_stream(amos_pnp *h) { return h ? (void *)h->stream : nullptr; }

int amos_pnp_ransac_device(amos_pnp *h, int n_problems, const float *d_object_xyz, const float *d_image_xy, const int32_t *d_offsets, const int32_t *d_counts,
                           const uint8_t *d_select, double fx, double fy, double cx, double cy, double reprojection_error, double confidence, int max_iters,
                           double *d_Rt, int32_t *d_status, uint8_t *d_mask)
{
    if (!h || n_problems < 0 || n_problems > h->maxProblems || !d_object_xyz || !d_image_xy || !d_counts || !d_Rt || !d_status ||
        !ransac_params_ok(reprojection_error, confidence, max_iters) || !camera_ok(fx, fy, cx, cy)) {
        set_error("amos_pnp_ransac_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    if (n_problems == 0) return AMOS_OK;
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    return pnp_launch(h, n_problems, d_object_xyz, d_image_xy, d_offsets, d_counts, d_select, fx, fy, cx, cy, reprojection_error, confidence, max_iters, d_Rt,
                      d_status, d_mask);
}

int amos_pnp_scene_flow_device(amos_pnp *h, const float *d_pre_xy, const float *d_next_xy, const uint8_t *d_state, const int32_t *d_n,
                               const float *d_depth_last, size_t last_stride, const float *d_depth_cur, size_t cur_stride, int width, int height,
                               const amos_scene_flow_camera *cam, double fx, double fy, double *d_Rt, int32_t *d_status, uint8_t *d_mask)
{
    if (!h || !d_pre_xy || !d_next_xy || !d_state || !d_n || !d_depth_last || !d_depth_cur || !cam || !d_Rt || !d_status || width < 1 || height < 1 ||
        last_stride < (size_t)width || cur_stride < (size_t)width || !camera_ok(fx, fy, cam->cx, cam->cy)) {
        set_error("amos_pnp_scene_flow_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    const SceneFlowArgs sa = scene_flow_args(cam);
    hipLaunchKernelGGL(k_pnp_points, dim3((h->maxPoints + 255) / 256), dim3(256), 0, h->stream, (const float2 *)d_pre_xy, (const float2 *)d_next_xy, d_n,
                       h->maxPoints, d_depth_last, last_stride, d_depth_cur, cur_stride, width, height, sa, h->dObj, h->dImg);
    AMOS_HIP_CHECK(hipGetLastError());
    // camera_mat of Tracking.cc:999-1004: fx, fy, cx, cy of mK (floats) as doubles; 500 iterations, 0.4 px, confidence 0.98
    return pnp_launch(h, 1, h->dObj, h->dImg, h->dInt, d_n, d_state, fx, fy, (double)cam->cx, (double)cam->cy, 0.4, 0.98, 500, d_Rt, d_status, d_mask);
}

int amos_pnp_ransac(amos_pnp *h, int n, const float *object_xyz, const float *image_xy, double fx, double fy, double cx, double cy, double reprojection_error,
                    double confidence, int max_iters, double *Rt, uint8_t *mask, int32_t *status)
{
    if (!h || n < 0 || n > h->maxPoints || (n > 0 && (!object_xyz || !image_xy)) || !Rt || !status || !ransac_params_ok(reprojection_error, confidence, max_iters) ||
        !camera_ok(fx, fy, cx, cy)) {
        set_error("amos_pnp_ransac: invalid argument (n <= max_points)");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    if (n > 0) {
        AMOS_HIP_CHECK(hipMemcpyAsync(h->dObj, object_xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, h->stream));
        AMOS_HIP_CHECK(hipMemcpyAsync(h->dImg, image_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, h->stream));
    }
    AMOS_HIP_CHECK(hipMemcpyAsync(h->dInt + 1, &n, sizeof(int), hipMemcpyHostToDevice, h->stream));
    const int rc = pnp_launch(h, 1, h->dObj, h->dImg, h->dInt, h->dInt + 1, nullptr, fx, fy, cx, cy, reprojection_error, confidence, max_iters, h->dRt, h->dInt + 2,
                              h->dMask);
    if (rc != AMOS_OK) return rc;
    AMOS_HIP_CHECK(hipMemcpyAsync(Rt, h->dRt, sizeof(double) * 12, hipMemcpyDeviceToHost, h->stream));
    AMOS_HIP_CHECK(hipMemcpyAsync(status, h->dInt + 2, sizeof(int) * kPnpStatus, hipMemcpyDeviceToHost, h->stream));
    if (mask && n > 0) AMOS_HIP_CHECK(hipMemcpyAsync(mask, h->dMask, n, hipMemcpyDeviceToHost, h->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(h->stream));
    return AMOS_OK;
}

}  // extern "C"
