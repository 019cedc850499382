// amos_dyna.hip -- the dynamic-object test of Amos-SLAM after the RANSACs: the tail of Tracking::GetSceneFlowObj (src/Tracking.cc:
// 1012-1184) and the decision of Frame::CalDyna (src/Frame.cc:552-628), so that the chain GetSceneFlowObj -> cluster -> decision ->
// labelled gate -> describe needs no host synchronisation.  The per-point arithmetic is amos_dyna.h and amos_scene_flow.h (restated:
// DESIGN.md section 2), the compaction and the sums amos_block.h.
//   k_dyna_tail    ONE WORK-GROUP PER CALL, 256 threads, n <= max_points (<= 4096).  Order-preserving compactions (the N-point lists,
//                  mvMatch / mvRpe, T_M, vFlow_3d) by a work-group prefix scan (ballot + per-wave counts, no atomics); both poses' errors
//                  in parallel; the inlier counts by a reduction; the pose choice and SetPose on one lane; then the scene flow under the
//                  chosen pose.
//   k_dyna_decide  ONE WORK-GROUP PER FRAME of a batch.  Cluster ids of the mvMatch entries in parallel; every cluster's Rpe sum on one
//                  lane walking the list in order (the reference's sequential float sum: no tree reduction); the distinct T_M
//                  superpixels through an LDS bitmap over the labels; epNum by integer LDS atomics (order-free); rm, AveClusterRpe, epNum.
#include "amos_common.h"
#include "amos_block.h"
#include "amos_dyna.h"

#include <cstddef>

namespace amos {

constexpr int kDynaMaxPoints = 4096;
constexpr int kDynaThreads = 256, kDynaWaves = kDynaThreads / 64;
constexpr int kDynaMaxCenters = 1 << 16;  // the decide bitmap (8 KB); 12 288 centres at 640 x 480 with len 5
constexpr int kDynaMaxCorners = 1000;     // goodFeaturesToTrack's maxCorners (Tracking.cc:894)
constexpr int kRecInts = (int)(sizeof(amos_slic_center) / sizeof(int32_t));
constexpr int kIdInt = (int)(offsetof(amos_slic_center, id) / sizeof(int32_t));

struct DynaSlot {  // the outputs of one slot
    float *pose, *rwc, *ow;
    int *choice, *counts;
    float2 *match;
    float *rpe;
    double *epi;
    float2 *tm;
    float *flow;
    int *status;
};

struct DynaTailArgs {
    const float2 *pre, *next;
    const uint8_t *state;
    const int *dN;
    int maxPoints;
    const double *F2, *Rt;
    const int *fmatStatus, *pnpStatus;
    const float *depthLast, *depthCur;
    size_t lastStride, curStride;
    int width, height;
    SceneFlowArgs sa;
    double fx, fy, cx, cy;
    float motion[12], lk[12];
    int hasLk;
    DynaSlot o;
};

__global__ __launch_bounds__(kDynaThreads) void k_dyna_tail(const DynaTailArgs a)
{
    __shared__ uint16_t sIdx[kDynaMaxPoints];  // tracked index of list entry j
    __shared__ float sRpeP[kDynaMaxPoints], sRpeM[kDynaMaxPoints];
    __shared__ float sScore[12], sMotion[12], sPose[12], sRwc[9], sOw[3];
    __shared__ int sWave[kDynaWaves], sChoice;
    const int t = threadIdx.x;
    const DynaSlot &o = a.o;
    const int n = *a.dN;
    int flags = (a.pnpStatus[0] != 1 ? AMOS_DYNA_NO_PNP : 0) | (a.fmatStatus[4] != 1 ? AMOS_DYNA_NO_F2 : 0);
    if (n < 0 || n > a.maxPoints) {
        if (t < AMOS_DYNA_COUNTS) o.counts[t] = 0;
        if (t < 12) o.pose[t] = 0.f;
        if (t < 9) o.rwc[t] = 0.f;
        if (t < 3) o.ow[t] = 0.f;
        if (t == 0) { *o.choice = 0; *o.status = flags | AMOS_DYNA_BAD_N; }
        return;
    }
    if (t < 12) {
        // Mod.at<float>(r, c) = d(r, c), Mod.at<float>(r, 3) = Tvec(r) (:1016-1018); the scoring pose of loop 1 is computeMtcwUseLK's mTcw if any
        const float mod = (float)(t % 4 == 3 ? a.Rt[9 + t / 4] : a.Rt[3 * (t / 4) + t % 4]);
        sPose[t] = mod;
        sScore[t] = a.hasLk ? a.lk[t] : mod;
        sMotion[t] = a.motion[t];
    }
    // ---- the N-point lists: the tracked points with state != 0, in order
    const int N = block_compact<kDynaThreads>(n, sWave, [&](int i) { return a.state[i] != 0; }, [&](int i, int c) { if (c >= 0) sIdx[c] = (uint16_t)i; });
    const int W = a.width, H = a.height;
    // scene_flow_depths (amos_scene_flow.h) written out: through the shared helper, in every form tried, the compiler schedules this kernel
    // differently and the tail measured 23.3 us against 22.6 us (profiles/r07_ransac_core.txt); as written here the code is the parent's
    auto depths = [&](float2 P, float2 Q, float &z1, float &z2) {  // truncated coordinates; outside the maps: no depth
        const int x1 = (int)P.x, y1 = (int)P.y, x2 = (int)Q.x, y2 = (int)Q.y;
        const bool in1 = P.x >= 0 && P.y >= 0 && x1 < W && y1 < H, in2 = Q.x >= 0 && Q.y >= 0 && x2 < W && y2 < H;
        z1 = in1 ? a.depthLast[(size_t)y1 * a.lastStride + x1] : 0.f;
        z2 = in2 ? a.depthCur[(size_t)y2 * a.curStride + x2] : 0.f;
    };
    // ---- loops 1 and 2 (:1028-1110): the entries with pre_3d.z > 0 && cur_2d.x != 0 && cur_2d.y != 0, errors under both poses
    int inP = 0, inM = 0;
    const int V = block_compact<kDynaThreads>(N, sWave,
        [&](int j) {
            const int i = sIdx[j];
            const float2 P = a.pre[i], Q = a.next[i];
            float z1, z2;
            depths(P, Q, z1, z2);
            if (!(z1 > 0 && z2 > 0)) return false;  // (0, 0, 0) -> (0, 0): pre_3d.z == 0
            float p0, p1, p2;
            scene_flow_pre3d(a.sa, P.x, P.y, z1, p0, p1, p2);
            return p2 > 0 && Q.x != 0 && Q.y != 0;
        },
        [&](int j, int c) {
            if (c < 0) return;
            const int i = sIdx[j];
            const float2 P = a.pre[i], Q = a.next[i];
            float z1, z2;
            depths(P, Q, z1, z2);
            float p0, p1, p2;
            scene_flow_pre3d(a.sa, P.x, P.y, z1, p0, p1, p2);
            const float eP = dyna::rpe(sScore, p0, p1, p2, Q.x, Q.y, a.fx, a.fy, a.cx, a.cy);
            const float eM = dyna::rpe(sMotion, p0, p1, p2, Q.x, Q.y, a.fx, a.fy, a.cx, a.cy);
            sRpeP[c] = eP;
            sRpeM[c] = eM;
            o.match[c] = Q;
            inP += (double)eP <= 0.4 ? 1 : 0;  // Rpe <= reprojectionError
            inM += (double)eM <= 0.4 ? 1 : 0;
        });
    const int nP = block_sum<kDynaThreads>(inP, sWave), nM = block_sum<kDynaThreads>(inM, sWave);
    // ---- the choice (:1112-1123) and SetPose
    if (t == 0) {
        const int choice = nP >= nM ? 1 : 0;
        if (!choice) for (int k = 0; k < 12; k++) sPose[k] = sMotion[k];
        dyna::set_pose(sPose, sRwc, sOw);
        sChoice = choice;
    }
    __syncthreads();
    const int choice = sChoice;
    if (t < 12) o.pose[t] = sPose[t];
    if (t < 9) o.rwc[t] = sRwc[t];
    if (t < 3) o.ow[t] = sOw[t];
    for (int c = t; c < V; c += kDynaThreads) o.rpe[c] = choice ? sRpeP[c] : sRpeM[c];
    // ---- mvepipolar and T_M under F2 (:1129-1145)
    double F[9];
    for (int k = 0; k < 9; k++) F[k] = a.F2[k];
    const int T = block_compact<kDynaThreads>(n, sWave,
        [&](int i) {
            if (a.state[i] == 0) return false;
            const float2 P = a.pre[i], Q = a.next[i];
            return !(epipolar_distance(F, P.x, P.y, Q.x, Q.y) <= 1.0);
        },
        [&](int i, int c) {
            const float2 P = a.pre[i], Q = a.next[i];
            o.epi[i] = a.state[i] != 0 ? epipolar_distance(F, P.x, P.y, Q.x, Q.y) : 0.0;
            if (c >= 0) o.tm[c] = Q;
        });
    // ---- vFlow_3d under the chosen pose (:1148-1183)
    float Rwc[9], Ow[3];
    for (int k = 0; k < 9; k++) Rwc[k] = sRwc[k];
    for (int k = 0; k < 3; k++) Ow[k] = sOw[k];
    auto flow_of = [&](int j, float &sf) {
        const int i = sIdx[j];
        const float2 P = a.pre[i], Q = a.next[i];
        float z1, z2;
        depths(P, Q, z1, z2);
        if (!(z1 > 0 && z2 > 0)) return false;
        sf = dyna::sf_norm(a.sa, Rwc, Ow, P.x, P.y, Q.x, Q.y, z1, z2);
        return sf > 3.f;
    };
    const int Fl = block_compact<kDynaThreads>(N, sWave, [&](int j) { float sf; return flow_of(j, sf); },
        [&](int j, int c) {
            if (c < 0) return;
            float sf;
            flow_of(j, sf);
            const float2 Q = a.next[sIdx[j]];
            o.flow[3 * c] = Q.x; o.flow[3 * c + 1] = Q.y; o.flow[3 * c + 2] = sf;
        });
    if (t == 0) {
        o.counts[0] = N; o.counts[1] = V; o.counts[2] = nP; o.counts[3] = nM; o.counts[4] = T; o.counts[5] = Fl;
        *o.choice = choice;
        *o.status = flags;
    }
}

// the first frame (Tracking.cc:377): empty lists
__global__ void k_dyna_reset(const DynaSlot o)
{
    const int t = threadIdx.x;
    if (t < AMOS_DYNA_COUNTS) o.counts[t] = 0;
    if (t < 12) o.pose[t] = 0.f;
    if (t < 9) o.rwc[t] = 0.f;
    if (t < 3) o.ow[t] = 0.f;
    if (t == 0) { *o.choice = 0; *o.status = AMOS_DYNA_RESET; }
}

struct DynaDecideArgs {
    const double *labels;
    size_t labelFrame, labelRow;
    int width, height;
    const int *centers;  // amos_slic_center records as int32
    size_t centerFrame;  // records
    int nCenters, k;
    int *rm;
    size_t rmFrame;
    // slot arrays
    const int *counts;
    const float2 *match, *tm;
    const float *rpe;
    int maxPoints;
    float *ave;
    int *ep, *status;
};

__global__ __launch_bounds__(kDynaThreads) void k_dyna_decide(const DynaDecideArgs a)
{
    __shared__ int8_t sCid[kDynaMaxPoints];
    __shared__ float sRpe[kDynaMaxPoints];
    __shared__ uint32_t sBits[kDynaMaxCenters / 32];
    __shared__ int sEp[AMOS_DYNA_MAX_K], sFlags;
    const int f = blockIdx.x, t = threadIdx.x;
    const int *cnt = a.counts + (size_t)f * AMOS_DYNA_COUNTS;
    const int V = min(max(cnt[1], 0), a.maxPoints), T = min(max(cnt[4], 0), a.maxPoints);
    const size_t so = (size_t)f * a.maxPoints;
    const double *labels = a.labels + (size_t)f * a.labelFrame;
    const int *centers = a.centers + (size_t)f * a.centerFrame * kRecInts;
    const int words = (a.nCenters + 31) >> 5;
    // (int) labelMask.at<double>((int) y, (int) x); 0 where the label is outside [1, n_centers] or the point outside the map
    auto label_of = [&](float2 P) {
        const int x = (int)P.x, y = (int)P.y;
        if (!(P.x >= 0 && P.y >= 0 && x < a.width && y < a.height)) return 0;
        const double l = labels[(size_t)y * a.labelRow + x];
        return l >= 1.0 && l <= (double)a.nCenters ? (int)l : 0;
    };
    if (t == 0) sFlags = 0;
    if (t < AMOS_DYNA_MAX_K) sEp[t] = 0;
    for (int w = t; w < words; w += kDynaThreads) sBits[w] = 0u;
    __syncthreads();
    int flags = 0;
    for (int j = t; j < V; j += kDynaThreads) {  // clusterRpe[centers[pixelId - 1].id] of mvMatch[j]
        const int l = label_of(a.match[so + j]);
        int id = -1;
        if (l == 0) flags |= AMOS_DYNA_BAD_MATCH_LABEL;
        else {
            id = centers[(size_t)(l - 1) * kRecInts + kIdInt];
            if (id < 0 || id >= a.k) { flags |= AMOS_DYNA_BAD_ID; id = -1; }
        }
        sCid[j] = (int8_t)id;
        sRpe[j] = a.rpe[so + j];
    }
    for (int j = t; j < T; j += kDynaThreads) {  // labelset of T_M
        const int l = label_of(a.tm[so + j]);
        if (l == 0) flags |= AMOS_DYNA_BAD_TM_LABEL;
        else atomicOr(&sBits[(l - 1) >> 5], 1u << ((l - 1) & 31));
    }
    __syncthreads();
    float ave = 0.f;
    if (t < 64) {  // wave 0: cluster t's sum, sequential in list order
        float sum = 0.f;
        int count = 0;
        for (int j = 0; j < V; j++) {
            if (sCid[j] == t) { sum = __fadd_rn(sum, sRpe[j]); count++; }
        }
        ave = __fdiv_rn(sum, (float)count);  // an empty cluster: 0 / 0 = NaN
    } else {  // waves 1..3: epNum[centers[label - 1].id]++ over the distinct labels
        for (int w = t - 64; w < words; w += kDynaThreads - 64) {
            uint32_t b = sBits[w];
            while (b) {
                const int l = (w << 5) + __ffs(b) - 1;  // label - 1
                b &= b - 1u;
                const int id = centers[(size_t)l * kRecInts + kIdInt];
                if (id < 0 || id >= a.k) flags |= AMOS_DYNA_BAD_ID;
                else atomicAdd(&sEp[id], 1);
            }
        }
    }
    if (flags) atomicOr(&sFlags, flags);
    __syncthreads();
    if (t < a.k) {
        const int ep = sEp[t];
        a.rm[(size_t)f * a.rmFrame + t] = ep > 0 && ave >= 3.f ? 1 : 0;
        a.ave[(size_t)f * AMOS_DYNA_MAX_K + t] = ave;
        a.ep[(size_t)f * AMOS_DYNA_MAX_K + t] = ep;
    }
    if (t == 0) a.status[f] = sFlags;
}

}  // namespace amos

using namespace amos;

struct amos_dyna : StreamHandle {
    int maxPoints = 0, maxFrames = 0;
    void *mem = nullptr;
    amos_dyna_results r{};
    uint8_t *lkStatus = nullptr, *keep = nullptr;
};

static DynaSlot dyna_slot(const amos_dyna *h, int f)
{
    const amos_dyna_results &r = h->r;
    const size_t P = (size_t)h->maxPoints;
    DynaSlot o;
    o.pose = r.pose + 12 * f; o.rwc = r.rwc + 9 * f; o.ow = r.ow + 3 * f;
    o.choice = r.choice + f; o.counts = r.counts + AMOS_DYNA_COUNTS * f;
    o.match = (float2 *)(r.match_xy + 2 * P * f);
    o.rpe = r.rpe + P * f;
    o.epi = r.epipolar + P * f;
    o.tm = (float2 *)(r.tm_xy + 2 * P * f);
    o.flow = r.flow + 3 * P * f;
    o.status = r.status + f;
    return o;
}

extern "C" {

int amos_dyna_create(int device, void *stream, int max_points, int max_frames, amos_dyna **out)
{
    if (!out || max_points < 1 || max_points > kDynaMaxPoints || max_frames < 1 || max_frames > 65535) {
        set_error("amos_dyna_create: invalid argument (1 <= max_points <= %d, 1 <= max_frames <= 65535)", kDynaMaxPoints);
        return AMOS_ERR_INVALID;
    }
    *out = nullptr;
    amos_dyna *h = new amos_dyna();
    h->maxPoints = max_points; h->maxFrames = max_frames;
    const int rc = h->open(device, stream);
    if (rc != AMOS_OK) { delete h; return rc; }
    // one allocation, every array 256-byte aligned
    const size_t P = (size_t)max_points, Fr = (size_t)max_frames;
    size_t off = 0;
    struct Part { void **p; size_t bytes; };
    amos_dyna_results &r = h->r;
    Part parts[] = {
        {(void **)&r.pose, sizeof(float) * 12 * Fr}, {(void **)&r.rwc, sizeof(float) * 9 * Fr}, {(void **)&r.ow, sizeof(float) * 3 * Fr},
        {(void **)&r.choice, sizeof(int32_t) * Fr}, {(void **)&r.counts, sizeof(int32_t) * AMOS_DYNA_COUNTS * Fr},
        {(void **)&r.match_xy, sizeof(float) * 2 * P * Fr}, {(void **)&r.rpe, sizeof(float) * P * Fr}, {(void **)&r.epipolar, sizeof(double) * P * Fr},
        {(void **)&r.tm_xy, sizeof(float) * 2 * P * Fr}, {(void **)&r.flow, sizeof(float) * 3 * P * Fr}, {(void **)&r.status, sizeof(int32_t) * Fr},
        {(void **)&r.ave_rpe, sizeof(float) * AMOS_DYNA_MAX_K * Fr}, {(void **)&r.ep_num, sizeof(int32_t) * AMOS_DYNA_MAX_K * Fr},
        {(void **)&r.decide_status, sizeof(int32_t) * Fr},
        {(void **)&r.pre_xy, sizeof(float) * 2 * P}, {(void **)&r.next_xy, sizeof(float) * 2 * P}, {(void **)&r.state, P}, {(void **)&r.n, sizeof(int32_t)},
        {(void **)&r.F1, sizeof(double) * 9}, {(void **)&r.F2, sizeof(double) * 9}, {(void **)&r.fmat_status, sizeof(int32_t) * 8},
        {(void **)&r.Rt, sizeof(double) * 12}, {(void **)&r.pnp_status, sizeof(int32_t) * 5},
        {(void **)&h->lkStatus, P}, {(void **)&h->keep, P},
    };
    for (const Part &q : parts) off += (q.bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(&h->mem, off);
    if (e == hipSuccess) e = hipMemsetAsync(h->mem, 0, off, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { set_error("amos_dyna_create: %s", hipGetErrorString(e)); amos_dyna_destroy(h); return AMOS_ERR_DEVICE; }
    off = 0;
    for (const Part &q : parts) {
        *q.p = (uint8_t *)h->mem + off;
        off += (q.bytes + 255) & ~(size_t)255;
    }
    r.max_points = max_points; r.max_frames = max_frames;
    *out = h;
    return AMOS_OK;
}

void amos_dyna_destroy(amos_dyna *h)
{
    if (!h) return;
    h->close();
    if (h->mem) (void)hipFree(h->mem);
    delete h;
}

void *amos_dyna_stream(amos_dyna *h) { return h ? (void *)h->stream : nullptr; }

int amos_dyna_results_device(amos_dyna *h, amos_dyna_results *out)
{
    if (!h || !out) { set_error("amos_dyna_results_device: invalid argument"); return AMOS_ERR_INVALID; }
    *out = h->r;
    return AMOS_OK;
}

int amos_dyna_copy_to_host(amos_dyna *h, void *dst, const void *d_src, size_t bytes)
{
    if (!h || (bytes && (!dst || !d_src))) { set_error("amos_dyna_copy_to_host: invalid argument"); return AMOS_ERR_INVALID; }
    if (!bytes) return AMOS_OK;
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    AMOS_HIP_CHECK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(h->stream));
    return AMOS_OK;
}

int amos_dyna_tail_device(amos_dyna *h, int frame, const float *d_pre_xy, const float *d_next_xy, const uint8_t *d_state, const int32_t *d_n,
                          const double *d_F2, const int32_t *d_fmat_status, const double *d_Rt, const int32_t *d_pnp_status,
                          const float *d_depth_last, size_t last_stride, const float *d_depth_cur, size_t cur_stride, int width, int height,
                          const amos_scene_flow_camera *cam, double fx, double fy, const amos_dyna_poses *poses)
{
    if (!h || frame < 0 || frame >= h->maxFrames || !d_pre_xy || !d_next_xy || !d_state || !d_n || !d_F2 || !d_fmat_status || !d_Rt || !d_pnp_status ||
        !d_depth_last || !d_depth_cur || width < 1 || height < 1 || last_stride < (size_t)width || cur_stride < (size_t)width || !poses ||
        !cam || !camera_ok(fx, fy, cam->cx, cam->cy)) {
        set_error("amos_dyna_tail_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    DynaTailArgs a;
    a.pre = (const float2 *)d_pre_xy; a.next = (const float2 *)d_next_xy; a.state = d_state; a.dN = d_n; a.maxPoints = h->maxPoints;
    a.F2 = d_F2; a.Rt = d_Rt; a.fmatStatus = d_fmat_status; a.pnpStatus = d_pnp_status;
    a.depthLast = d_depth_last; a.depthCur = d_depth_cur; a.lastStride = last_stride; a.curStride = cur_stride;
    a.width = width; a.height = height;
    a.sa = scene_flow_args(cam);
    a.fx = fx; a.fy = fy; a.cx = (double)cam->cx; a.cy = (double)cam->cy;  // camera_mat of Tracking.cc:999-1004
    for (int k = 0; k < 12; k++) { a.motion[k] = poses->motion[k]; a.lk[k] = poses->lk[k]; }
    a.hasLk = poses->has_lk != 0;
    a.o = dyna_slot(h, frame);
    hipLaunchKernelGGL(k_dyna_tail, dim3(1), dim3(kDynaThreads), 0, h->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_dyna_reset_frame_device(amos_dyna *h, int frame)
{
    if (!h || frame < 0 || frame >= h->maxFrames) { set_error("amos_dyna_reset_frame_device: invalid argument"); return AMOS_ERR_INVALID; }
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_dyna_reset, dim3(1), dim3(64), 0, h->stream, dyna_slot(h, frame));
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_dyna_decide_batch_device(amos_dyna *h, int n_frames, const double *d_labels, size_t label_frame_stride, size_t label_row_stride, int width,
                                  int height, const amos_slic_center *d_centers, size_t centers_frame_stride, int n_centers, int k, int32_t *d_rm,
                                  size_t rm_frame_stride)
{
    if (!h || n_frames < 0 || n_frames > h->maxFrames || !d_labels || !d_centers || !d_rm || width < 1 || height < 1 ||
        label_row_stride < (size_t)width || n_centers < 1 || n_centers > kDynaMaxCenters || k < 1 || k > AMOS_DYNA_MAX_K ||
        (n_frames > 1 && (label_frame_stride < label_row_stride * height || centers_frame_stride < (size_t)n_centers || rm_frame_stride < (size_t)k))) {
        set_error("amos_dyna_decide_batch_device: invalid argument (n_frames <= max_frames, 1 <= k <= %d, 1 <= n_centers <= %d)", AMOS_DYNA_MAX_K,
                  kDynaMaxCenters);
        return AMOS_ERR_INVALID;
    }
    if (n_frames == 0) return AMOS_OK;
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    DynaDecideArgs a;
    a.labels = d_labels; a.labelFrame = label_frame_stride; a.labelRow = label_row_stride;
    a.width = width; a.height = height;
    a.centers = (const int *)d_centers; a.centerFrame = centers_frame_stride;
    a.nCenters = n_centers; a.k = k;
    a.rm = d_rm; a.rmFrame = rm_frame_stride;
    a.counts = h->r.counts; a.match = (const float2 *)h->r.match_xy; a.tm = (const float2 *)h->r.tm_xy; a.rpe = h->r.rpe;
    a.maxPoints = h->maxPoints;
    a.ave = h->r.ave_rpe; a.ep = h->r.ep_num; a.status = h->r.decide_status;
    hipLaunchKernelGGL(k_dyna_decide, dim3(n_frames), dim3(kDynaThreads), 0, h->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_dyna_scene_flow_obj_device(amos_dyna *h, int frame, amos_corners *corners, amos_lk *lk, amos_fmat *fmat, amos_pnp *pnp,
                                    const uint8_t *d_imlast_gray, size_t last_gray_stride, const uint8_t *d_gray, size_t gray_stride, int width,
                                    int height, const float *d_depth_last, size_t last_stride, const float *d_depth_cur, size_t cur_stride,
                                    const amos_scene_flow_camera *cam, double fx, double fy, const amos_dyna_poses *poses)
{
    if (!h || frame < 0 || frame >= h->maxFrames || !corners || !lk || !fmat || !pnp || !d_imlast_gray || !d_gray || !d_depth_last || !d_depth_cur ||
        width < 1 || height < 1 || last_gray_stride < (size_t)width || gray_stride < (size_t)width || last_stride < (size_t)width ||
        cur_stride < (size_t)width || !poses || !cam || !camera_ok(fx, fy, cam->cx, cam->cy)) {
        set_error("amos_dyna_scene_flow_obj_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    if (amos_corners_stream(corners) != (void *)h->stream || amos_lk_stream(lk) != (void *)h->stream || amos_fmat_stream(fmat) != (void *)h->stream ||
        amos_pnp_stream(pnp) != (void *)h->stream) {
        set_error("amos_dyna_scene_flow_obj_device: the corner, LK, fmat and PnP handles must use the dyna handle's stream");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(h->device));
    const amos_dyna_results &r = h->r;
    const int nc = h->maxPoints < kDynaMaxCorners ? h->maxPoints : kDynaMaxCorners;
    AMOS_HIP_CHECK(hipMemsetAsync(r.pre_xy, 0, sizeof(float) * 2 * nc, h->stream));
    int rc = amos_corners_good_features_device(corners, d_imlast_gray, last_gray_stride, width, height, nc, 0.01, 8.0, 0.04, r.pre_xy, nc, r.n, nullptr);
    if (rc == AMOS_OK) rc = amos_corners_subpix_device(corners, d_imlast_gray, last_gray_stride, width, height, r.pre_xy, r.n, nc, 10, 20, 0.03);
    if (rc == AMOS_OK)
        rc = amos_lk_track_device(lk, d_imlast_gray, last_gray_stride, d_gray, gray_stride, r.pre_xy, nc, 20, 0.01, 1e-4f, r.next_xy, h->lkStatus, nullptr);
    if (rc == AMOS_OK)
        rc = amos_flow_check_device(h->stream, d_imlast_gray, last_gray_stride, d_gray, gray_stride, width, height, r.pre_xy, r.next_xy, h->lkStatus, nc,
                                    r.state);
    if (rc == AMOS_OK) rc = amos_fmat_scene_flow_pair_device(fmat, r.pre_xy, r.next_xy, r.state, r.n, r.F1, r.F2, h->keep, r.fmat_status);
    if (rc == AMOS_OK)
        rc = amos_pnp_scene_flow_device(pnp, r.pre_xy, r.next_xy, r.state, r.n, d_depth_last, last_stride, d_depth_cur, cur_stride, width, height, cam, fx,
                                        fy, r.Rt, r.pnp_status, nullptr);
    if (rc == AMOS_OK)
        rc = amos_dyna_tail_device(h, frame, r.pre_xy, r.next_xy, r.state, r.n, r.F2, r.fmat_status, r.Rt, r.pnp_status, d_depth_last, last_stride,
                                   d_depth_cur, cur_stride, width, height, cam, fx, fy, poses);
    return rc;
}

}  // extern "C"
