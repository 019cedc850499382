// amos_stereo.hip -- Frame::ComputeStereoMatches (Frame.cc:1179-1573) on the device, for pairs of resident extractions: the band search
// over the right keypoints with its Hamming loop, the 11 x 11 SAD refinement over 11 shifts, the parabola fit and the depth (k_stereo_match,
// one wave per left keypoint), then the median rejection (k_stereo_median, one work-group per pair).  Integer Hamming and SAD, a handful of
// float32 operations in the source's order (explicit _rn intrinsics, nothing fused): the same bits as the sequential routine.
// Parity with the reference's shipped binary is unpinned (DESIGN.md "Stereo matching"): whether its -O3 -march=native build contracted
// uL - scale * (...) into one FMA is unknown; the definition here is the unfused source.
#include "amos_block.h"

#include <cstdint>
#include <cstring>

namespace amos {

constexpr int kStereoWaves = 4;                  // left keypoints per work-group of k_stereo_match
constexpr int kStereoThreads = 64 * kStereoWaves;
constexpr int kStereoW = 5, kStereoL = 5;        // Frame.cc:1393,1414: window half size, shift range
constexpr int kStereoWin = 2 * kStereoW + 1;     // 11
constexpr int kStereoStrip = kStereoWin + 2 * kStereoL;  // 21 columns of the right strip
constexpr int kStereoKeyShift = 22;              // arg-min key = dist << 22 | iR: right capacities below 2^22
constexpr int kMedianThreads = 256;

struct StereoArgs {
    const Geom *geom;                  // the (common) level geometry
    const uint8_t *pyrL, *pyrR;        // padded pyramid planes, frame f at + f * frameBytes
    unsigned long long frameBytes;
    const amos_keypoint *kpsL, *kpsR;  // [frames][capL] / [frames][capR]
    const uint8_t *descL, *descR;      // 32-byte rows, 16-byte aligned
    const int *countsL, *countsR;      // [frames]
    int capL, capR;
    int frameMul, frameOffR;           // pair p: left frame p * frameMul, right frame p * frameMul + frameOffR
    int nLevels, nRows;                // nRows = mvImagePyramid[0].rows
    float mbf, maxD;                   // maxD = mbf / minZ (Frame.cc:1272)
    float scale[AMOS_MAX_LEVELS], invScale[AMOS_MAX_LEVELS];
    float *uRight, *depth;             // [pairs][capL]
    int *sad;                          // [pairs][capL]
    int *status;                       // [pairs] or nullptr
};

// Pixel (x, y) of a level (level coordinates) in its padded plane.  The reference takes its windows with rowRange / colRange and checks
// neither rows nor the left window's columns (Frame.cc:1401,1434); the resident planes carry the 19-px reflect-101 border of
// mvImagePyramid, and the index is CLAMPED into that padded plane so that no read leaves the allocation whatever the keypoint holds.
__device__ __forceinline__ int plane_px(const uint8_t *plane, const LevelGeom &lg, int x, int y)
{
    x = min(max(x, -kEdge), lg.w + kEdge - 1);
    y = min(max(y, -kEdge), lg.h + kEdge - 1);
    return plane[(size_t)(y + kEdge) * lg.stride + kPadLeft + x];
}

// grid = (ceil(capL / kStereoWaves), pairs), block = kStereoThreads: wave w of the group owns left keypoint blockIdx.x * kStereoWaves + w.
__global__ __launch_bounds__(kStereoThreads) void k_stereo_match(const StereoArgs a)
{
    __shared__ float4 sRight[kStereoThreads];                              // (floor(y - r), ceil(y + r), octave bits, x) of a tile of right keypoints
    __shared__ uint8_t sWinL[kStereoWaves][kStereoWin * kStereoWin + 7];   // the left window, per wave
    __shared__ uint8_t sWinR[kStereoWaves][kStereoWin * kStereoStrip + 9]; // the right strip, per wave
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, pair = blockIdx.y;
    const int frameL = pair * a.frameMul, frameR = frameL + a.frameOffR;
    const int nL = min(max(a.countsL[frameL], 0), a.capL), nR = min(max(a.countsR[frameR], 0), a.capR);
    const int iL = blockIdx.x * kStereoWaves + wv;
    const size_t o = (size_t)pair * a.capL + iL;
    if (iL < a.capL && lane == 0) {  // Frame.cc:1184-1185: everything starts at -1 (the whole capacity row: the bytes are defined)
        a.uRight[o] = -1.f;
        a.depth[o] = -1.f;
        a.sad[o] = -1;
    }
    if (blockIdx.x * kStereoWaves >= nL) return;  // group-uniform: no barrier below is skipped by a part of the group

    // ---- the left keypoint (wave-uniform)
    amos_keypoint kpL{};
    bool live = iL < nL;
    if (live) kpL = a.kpsL[(size_t)frameL * a.capL + iL];
    const int levelL = kpL.octave;
    const float uL = kpL.x, vL = kpL.y;
    // vRowIndices[vL] (Frame.cc:1298): the row is (int) vL; a row outside [0, nRows) or an octave outside the pyramid never matches
    live = live && levelL >= 0 && levelL < a.nLevels && vL > -1.f && vL < (float)a.nRows;
    const float rowL = (float)(int)vL;
    const float minU = __fsub_rn(uL, a.maxD), maxU = uL;  // Frame.cc:1307-1308, minD = 0
    live = live && !(maxU < 0.f);                         // :1315
    uint32_t dl[8] = {};
    if (live) {
        const uint4 *p = reinterpret_cast<const uint4 *>(a.descL + ((size_t)frameL * a.capL + iL) * 32);
        const uint4 lo = p[0], hi = p[1];
        dl[0] = lo.x; dl[1] = lo.y; dl[2] = lo.z; dl[3] = lo.w; dl[4] = hi.x; dl[5] = hi.y; dl[6] = hi.z; dl[7] = hi.w;
    }

    // ---- band search, Frame.cc:1332-1369: candidates in ascending iR, the first strict minimum wins = minimum over (dist, iR)
    const uint32_t keyInit = (uint32_t)AMOS_TH_HIGH << kStereoKeyShift;
    uint32_t key = keyInit;
    for (int base = 0; base < nR; base += kStereoThreads) {
        {
            const int iR = base + t;
            float4 rec = make_float4(1.f, 0.f, __int_as_float(-8), 0.f);  // an empty band
            if (iR < nR) {
                const amos_keypoint kp = a.kpsR[(size_t)frameR * a.capR + iR];
                if (kp.octave >= 0 && kp.octave < a.nLevels) {
                    const float r = __fmul_rn(2.0f, a.scale[kp.octave]);  // :1239
                    rec = make_float4(floorf(__fsub_rn(kp.y, r)), ceilf(__fadd_rn(kp.y, r)), __int_as_float(kp.octave), kp.x);
                }
            }
            sRight[t] = rec;
        }
        __syncthreads();
        if (live) {
            const int n = min(kStereoThreads, nR - base);
            for (int j = lane; j < n; j += 64) {
                const float4 rec = sRight[j];
                const int octR = __float_as_int(rec.z);
                // a NaN coordinate fails every comparison: never a candidate
                if (!(rec.x <= rowL && rowL <= rec.y) || octR < levelL - 1 || octR > levelL + 1 || !(rec.w >= minU && rec.w <= maxU)) continue;
                const uint4 *p = reinterpret_cast<const uint4 *>(a.descR + ((size_t)frameR * a.capR + base + j) * 32);
                const uint4 lo = p[0], hi = p[1];
                const int dist = __popcll(((unsigned long long)(lo.y ^ dl[1]) << 32) | (lo.x ^ dl[0])) +
                                 __popcll(((unsigned long long)(lo.w ^ dl[3]) << 32) | (lo.z ^ dl[2])) +
                                 __popcll(((unsigned long long)(hi.y ^ dl[5]) << 32) | (hi.x ^ dl[4])) +
                                 __popcll(((unsigned long long)(hi.w ^ dl[7]) << 32) | (hi.z ^ dl[6]));
                key = min(key, ((uint32_t)dist << kStereoKeyShift) | (uint32_t)(base + j));
            }
        }
        __syncthreads();
    }
    for (int d = 32; d > 0; d >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, d, 64));
    const int bestDist = (int)(key >> kStereoKeyShift);
    live = live && bestDist < (AMOS_TH_HIGH + AMOS_TH_LOW) / 2;  // :1377 (key == keyInit: no candidate, bestDist == TH_HIGH)

    // ---- SAD refinement at the left keypoint's level, Frame.cc:1384-1459
    int cu = 0, cv = 0, cr = 0;
    float fr = 0.f;  // scaleduR0 as the float the source keeps
    if (live) {
        const int bestIdxR = (int)(key & ((1u << kStereoKeyShift) - 1u));
        const float uR0 = a.kpsR[(size_t)frameR * a.capR + bestIdxR].x;
        const float sf = a.invScale[levelL];
        const float scaleduL = roundf(__fmul_rn(uL, sf)), scaledvL = roundf(__fmul_rn(vL, sf)), scaleduR0 = roundf(__fmul_rn(uR0, sf));
        const float iniu = __fsub_rn(__fadd_rn(scaleduR0, (float)kStereoL), (float)kStereoW);         // :1422, the +L as written
        const float endu = __fadd_rn(__fadd_rn(__fadd_rn(scaleduR0, (float)kStereoL), (float)kStereoW), 1.f);  // :1423
        live = !(iniu < 0.f || endu >= (float)a.geom->lv[levelL].w);  // :1425 (NaN passes both comparisons as in the source; the clamps below hold)
        cu = (int)scaleduL;
        cv = (int)scaledvL;
        cr = (int)scaleduR0;
        fr = scaleduR0;
    }
    if (live) {
        const LevelGeom &lg = a.geom->lv[levelL];
        const uint8_t *pl = a.pyrL + (size_t)frameL * a.frameBytes + lg.planeOff, *pr = a.pyrR + (size_t)frameR * a.frameBytes + lg.planeOff;
        for (int k = lane; k < kStereoWin * kStereoWin; k += 64)
            sWinL[wv][k] = (uint8_t)plane_px(pl, lg, cu - kStereoW + k % kStereoWin, cv - kStereoW + k / kStereoWin);
        for (int k = lane; k < kStereoWin * kStereoStrip; k += 64)
            sWinR[wv][k] = (uint8_t)plane_px(pr, lg, cr - kStereoL - kStereoW + k % kStereoStrip, cv - kStereoW + k / kStereoStrip);
    }
    __syncthreads();  // every wave of the group arrives here (the windows are per wave; the barrier orders their LDS writes and reads)
    if (!live) return;
    int part[2 * kStereoL + 1] = {};
    {
        const int cL = sWinL[wv][kStereoW * kStereoWin + kStereoW];
        const uint8_t *rowC = &sWinR[wv][kStereoW * kStereoStrip];
        for (int k = lane; k < kStereoWin * kStereoWin; k += 64) {
            const int dy = k / kStereoWin, dx = k % kStereoWin;
            const int vl = (int)sWinL[wv][k] - cL;  // each window has its own centre pixel subtracted (:1405,1440)
            const uint8_t *row = &sWinR[wv][dy * kStereoStrip + dx];
#pragma unroll
            for (int s = 0; s <= 2 * kStereoL; s++) part[s] += abs(vl - ((int)row[s] - (int)rowC[s + kStereoW]));
        }
    }
    int bestSad = 0x7fffffff, bestInc = 0, dists[2 * kStereoL + 1];
#pragma unroll
    for (int s = 0; s <= 2 * kStereoL; s++) {
        dists[s] = wave_sum(part[s]);  // cv::norm(IL, IR, NORM_L1): an exact integer, at most 121 * 510
        if (dists[s] < bestSad) {      // :1449, the first smallest wins
            bestSad = dists[s];
            bestInc = s - kStereoL;
        }
    }
    if (bestInc == -kStereoL || bestInc == kStereoL) return;  // :1468

    // ---- parabola fit and depth, Frame.cc:1482-1533, float32 in source order
    float d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
    for (int s = 1; s < 2 * kStereoL; s++)
        if (s == bestInc + kStereoL) { d1 = (float)dists[s - 1]; d2 = (float)dists[s]; d3 = (float)dists[s + 1]; }
    const float deltaR = __fdiv_rn(__fsub_rn(d1, d3), __fmul_rn(2.0f, __fsub_rn(__fadd_rn(d1, d3), __fmul_rn(2.0f, d2))));
    if (deltaR < -1.f || deltaR > 1.f) return;  // :1499 (an infinite deltaR leaves here, a NaN at the next comparison)
    float bestuR = __fmul_rn(a.scale[levelL], __fadd_rn(__fadd_rn(fr, (float)bestInc), deltaR));  // :1509
    float disparity = __fsub_rn(uL, bestuR);
    if (!(disparity >= 0.f && disparity < a.maxD)) return;  // :1515
    if (disparity <= 0.f) {                                 // :1521-1525: double constants assigned to floats
        disparity = 0.01f;
        bestuR = (float)((double)uL - 0.01);
    }
    if (lane == 0) {
        a.depth[o] = __fdiv_rn(a.mbf, disparity);
        a.uRight[o] = bestuR;
        a.sad[o] = bestSad;
    }
}

// Frame.cc:1548-1569 for one pair per work-group: median = element count / 2 of the accepted SADs in ascending order (found by
// bisection on its bits over block sums: no sort, no atomics), thDist = 1.5f * 1.4f * median, every accepted keypoint with
// (float) sad >= thDist back to -1.  Also the pair's status word: bit 1 = a left keypoint's row or a keypoint's octave out of range.
__global__ __launch_bounds__(kMedianThreads) void k_stereo_median(const StereoArgs a)
{
    __shared__ int sWave[kMedianThreads / 64];
    const int t = threadIdx.x, pair = blockIdx.x;
    const int frameL = pair * a.frameMul, frameR = frameL + a.frameOffR;
    const int nL = min(max(a.countsL[frameL], 0), a.capL), nR = min(max(a.countsR[frameR], 0), a.capR);
    const int *sad = a.sad + (size_t)pair * a.capL;
    if (a.status) {
        int bad = 0;
        for (int i = t; i < nL; i += kMedianThreads) {
            const amos_keypoint kp = a.kpsL[(size_t)frameL * a.capL + i];
            bad |= !(kp.octave >= 0 && kp.octave < a.nLevels && kp.y > -1.f && kp.y < (float)a.nRows);
        }
        for (int i = t; i < nR; i += kMedianThreads) {
            const int oct = a.kpsR[(size_t)frameR * a.capR + i].octave;
            bad |= !(oct >= 0 && oct < a.nLevels);
        }
        bad = block_sum<kMedianThreads>(bad, sWave);
        if (t == 0) a.status[pair] = bad ? 1 : 0;
    }
    int mine = 0;
    for (int i = t; i < nL; i += kMedianThreads) mine += sad[i] >= 0;
    const int count = block_sum<kMedianThreads>(mine, sWave);
    if (count == 0) return;  // the reference indexes an empty vector here (:1549); defined as "nothing matched"
    const int k = count / 2;
    int median = 0;  // the largest m with #(sad < m) <= k is the k-th smallest; SADs are below 121 * 510 < 2^16
    for (int bit = 16; bit >= 0; bit--) {
        const int m = median | (1 << bit);
        int below = 0;
        for (int i = t; i < nL; i += kMedianThreads) below += sad[i] >= 0 && sad[i] < m;
        if (block_sum<kMedianThreads>(below, sWave) <= k) median = m;
    }
    const float thDist = __fmul_rn(1.5f * 1.4f, (float)median);  // :1551, the constant product formed in float32 first
    for (int i = t; i < nL; i += kMedianThreads)
        if (sad[i] >= 0 && !((float)sad[i] < thDist)) {  // :1560
            a.uRight[(size_t)pair * a.capL + i] = -1.f;
            a.depth[(size_t)pair * a.capL + i] = -1.f;
        }
}

static bool same_params(const amos_orb_params &x, const amos_orb_params &y)
{
    return x.n_features == y.n_features && x.scale_factor == y.scale_factor && x.n_levels == y.n_levels && x.ini_th_fast == y.ini_th_fast &&
           x.min_th_fast == y.min_th_fast;
}

}  // namespace amos

using namespace amos;

extern "C" {

int amos_frame_stereo_match_arrays_device(amos_orb *left, amos_orb *right, int n_pairs, const amos_keypoint *d_kps_l, const uint8_t *d_desc_l,
                                          const int32_t *d_counts_l, int capacity_l, const amos_keypoint *d_kps_r, const uint8_t *d_desc_r,
                                          const int32_t *d_counts_r, int capacity_r, float mbf, float min_z, float *d_u_right, float *d_depth,
                                          int32_t *d_sad, int32_t *d_status)
{
    const char *who = "amos_frame_stereo_match_arrays_device";
    if (!left || !right || n_pairs < 1 || !d_kps_l || !d_desc_l || !d_counts_l || !d_kps_r || !d_desc_r || !d_counts_r || !d_u_right || !d_depth) {
        set_error("%s: invalid argument (a handle, an input array or an output is NULL, or n_pairs < 1)", who);
        return AMOS_ERR_INVALID;
    }
    if (capacity_l < 1 || capacity_r < 1 || capacity_r >= (1 << kStereoKeyShift) || (((uintptr_t)d_desc_l | (uintptr_t)d_desc_r) & 15)) {
        set_error("%s: capacities must be 1 .. 2^22 - 1 and the descriptor arrays 16-byte aligned", who);
        return AMOS_ERR_INVALID;
    }
    if (!(mbf > 0.f) || !(min_z > 0.f)) { set_error("%s: mbf and min_z must be positive (got %g, %g)", who, (double)mbf, (double)min_z); return AMOS_ERR_INVALID; }
    const bool interleaved = left == right;
    OrbStereoView L, R;
    int rc = orb_stereo_view(left, d_sad == nullptr ? n_pairs * (size_t)capacity_l : 0, &L);
    if (rc != AMOS_OK) return rc;
    if (interleaved) R = L;
    else if ((rc = orb_stereo_view(right, 0, &R)) != AMOS_OK) return rc;
    if (!L.detected || !R.detected) { set_error("%s before an extraction", who); return AMOS_ERR_STATE; }
    if (L.device != R.device) { set_error("%s: the handles live on devices %d and %d", who, L.device, R.device); return AMOS_ERR_INVALID; }
    if (!same_params(L.p, R.p) || L.width != R.width || L.height != R.height) {
        set_error("%s: the handles differ in their extractor parameters or frame size (%dx%d, %dx%d)", who, L.width, L.height, R.width, R.height);
        return AMOS_ERR_INVALID;
    }
    if ((interleaved ? 2 * n_pairs : n_pairs) > L.nFrames || n_pairs > R.nFrames) {
        set_error("%s: %d pairs need more frames than the last batch holds (%d, %d)", who, n_pairs, L.nFrames, R.nFrames);
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(L.device));
    StereoArgs a{};
    a.geom = L.dGeom;
    a.pyrL = L.dPyr;
    a.pyrR = R.dPyr;
    a.frameBytes = L.frameBytes;
    a.kpsL = d_kps_l; a.descL = d_desc_l; a.countsL = d_counts_l; a.capL = capacity_l;
    a.kpsR = d_kps_r; a.descR = d_desc_r; a.countsR = d_counts_r; a.capR = capacity_r;
    a.frameMul = interleaved ? 2 : 1;
    a.frameOffR = interleaved ? 1 : 0;
    a.nLevels = L.p.n_levels;
    a.nRows = L.height;
    a.mbf = mbf;
    a.maxD = mbf / min_z;  // Frame.cc:1272, float32
    for (int l = 0; l < a.nLevels; l++) { a.scale[l] = L.scale[l]; a.invScale[l] = L.invScale[l]; }
    a.uRight = d_u_right;
    a.depth = d_depth;
    a.sad = d_sad ? d_sad : L.dSadScratch;
    a.status = d_status;
    if (!interleaved) {  // the right handle's extraction precedes the reads of its planes: an event, no host synchronisation
        AMOS_HIP_CHECK(hipEventRecord(R.event, R.stream));
        AMOS_HIP_CHECK(hipStreamWaitEvent(L.stream, R.event, 0));
    }
    hipLaunchKernelGGL(k_stereo_match, dim3((capacity_l + kStereoWaves - 1) / kStereoWaves, n_pairs), dim3(kStereoThreads), 0, L.stream, a);
    hipLaunchKernelGGL(k_stereo_median, dim3(n_pairs), dim3(kMedianThreads), 0, L.stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    if (!interleaved) {  // and the right handle's next extraction follows them
        AMOS_HIP_CHECK(hipEventRecord(L.event, L.stream));
        AMOS_HIP_CHECK(hipStreamWaitEvent(R.stream, L.event, 0));
    }
    return AMOS_OK;
}

int amos_frame_stereo_match_batch_device(amos_orb *left, amos_orb *right, int n_pairs, float mbf, float min_z, float *d_u_right, float *d_depth,
                                         int32_t *d_sad, int32_t *d_status)
{
    const char *who = "amos_frame_stereo_match_batch_device";
    if (!left || !right) { set_error("%s: invalid argument (a handle is NULL)", who); return AMOS_ERR_INVALID; }
    OrbStereoView L, R;
    int rc = orb_stereo_view(left, 0, &L);
    if (rc != AMOS_OK) return rc;
    if ((rc = orb_stereo_view(right, 0, &R)) != AMOS_OK) return rc;
    if (!L.described || !R.described) { set_error("%s before an extraction", who); return AMOS_ERR_STATE; }
    return amos_frame_stereo_match_arrays_device(left, right, n_pairs, L.dKps, L.dDesc, L.dCounts, L.capacity, R.dKps, R.dDesc, R.dCounts, R.capacity,
                                                 mbf, min_z, d_u_right, d_depth, d_sad, d_status);
}

int amos_frame_stereo_match(amos_orb *left, amos_orb *right, float mbf, float min_z, float *u_right, float *depth, int n)
{
    const char *who = "amos_frame_stereo_match";
    if (!left || !right || !u_right || !depth || n < 0) { set_error("%s: invalid argument", who); return AMOS_ERR_INVALID; }
    OrbStereoView L;
    int rc = orb_stereo_view(left, 0, &L);
    if (rc != AMOS_OK) return rc;
    if (n > L.capacity) { set_error("%s: %d keypoints asked for, the handle's capacity is %d", who, n, L.capacity); return AMOS_ERR_CAPACITY; }
    float *dU = L.dOutHostForm, *dD = L.dOutHostForm + L.capacity;
    rc = amos_frame_stereo_match_batch_device(left, right, 1, mbf, min_z, dU, dD, nullptr, nullptr);
    if (rc != AMOS_OK) return rc;
    // ONE device-to-host transfer: the two float arrays are adjacent
    AMOS_HIP_CHECK(hipMemcpyAsync(L.hStage, L.dOutHostForm, sizeof(float) * 2 * (size_t)L.capacity, hipMemcpyDeviceToHost, L.stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(L.stream));
    if (n > 0) {
        std::memcpy(u_right, L.hStage, sizeof(float) * n);
        std::memcpy(depth, L.hStage + sizeof(float) * (size_t)L.capacity, sizeof(float) * n);
    }
    return AMOS_OK;
}

}  // extern "C"
