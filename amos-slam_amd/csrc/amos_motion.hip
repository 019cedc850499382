// amos_motion.hip -- Tracking::TrackWithMotionModel's search (Tracking.cc:1925-1945) for a batch of resident frames: the fill of
// mvpMapPoints, ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1569-1728) and the second search with the
// doubled radius when the first found fewer than 20 matches.
//
// Launches on the matcher's stream: k_motion_project (one thread per last-frame point), k_motion_window_best2 (eight lanes per projected
// point: the best two features of its window in the EMPTY frame) and k_motion_accept (one wave per frame: the reference's sequential
// greedy loop over those records, then the rotation histogram's pruning); the last two once more with th_retry, where every work-group
// of a frame whose first search found enough returns at once.  The arithmetic is defined in include/amos_frontend.h, "motion-model search".
#include "amos_common.h"
#include "amos_match_core.h"
#include "amos_scene_flow.h"  // gemm_row

#include "../../include/amos_host_types.h"  // amos_proj_query

#include <climits>
#include <cmath>
#include <vector>

namespace amos {

static_assert(sizeof(amos_last_point) == 64, "amos_last_point is 64 bytes (include/amos_frontend.h)");
static_assert(sizeof(amos_motion_camera) == 140, "amos_motion_camera is 140 bytes");
static_assert(sizeof(amos_motion_stats) == 32, "amos_motion_stats is 32 bytes");
static_assert(sizeof(amos_proj_query) == 56, "amos_proj_query is 56 bytes");

struct MotionFrame {
    amos_motion_camera cam;
    int off0, off1;  // the frame's points
    int flags;       // bit 0 bForward, bit 1 bBackward
};

struct MotionArgs {
    const amos_keypoint *kps;
    const uint8_t *desc;
    const int *counts, *cellStart, *items;
    const float *uRight;
    const amos_last_point *points;
    const MotionFrame *frames;
    amos_proj_query *query;
    uint8_t *projected;
    int *match;
    amos_motion_stats *stats;
    amos_best2 *best2;  // scratch, one per point
    int *accepted;      // scratch, one per point: -1, or bin << 16 | feature of the point's accepted match
    uint8_t *flags;     // scratch, one per point: bit 0 projected, bit 1 a projection that is not finite, bit 2 an octave outside the table
    float scale[AMOS_MAX_LEVELS];
    float minX, maxX, minY, maxY, wInv, hInv;
    int capacity, nLevels;
    int pass;  // 1: radius th; 2: radius th_retry, for the frames whose first search stayed below retry_below
};

constexpr int kMotionTakenWords = 65536 / 32;

// ---- the projection of ORBmatcher.cc:1604-1626.  grid = (ceil(max points of a frame / 256), frames), block = 256.
__global__ __launch_bounds__(256) void k_motion_project(const MotionArgs a)
{
    const MotionFrame &fr = a.frames[blockIdx.y];
    const int p = fr.off0 + blockIdx.x * 256 + threadIdx.x;
    if (p >= fr.off1) return;
    const amos_motion_camera &c = fr.cam;
    const amos_last_point &lp = a.points[p];
    amos_proj_query q;
    q.u = q.v = q.invz = 0.f;
    q.octave = lp.octave;
    q.angle = lp.angle;
    q.has_obs = (lp.flags & AMOS_LAST_POINT_HAS_OBS) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 8; k++) reinterpret_cast<uint32_t *>(q.desc)[k] = reinterpret_cast<const uint32_t *>(lp.desc)[k];
    int flags = 0;
    if (!(lp.flags & AMOS_LAST_POINT_SKIP)) {
        const float P0 = lp.pos[0], P1 = lp.pos[1], P2 = lp.pos[2];
        const float xc = gemm_row(c.Rcw, 0, P0, P1, P2, c.tcw[0]);
        const float yc = gemm_row(c.Rcw, 1, P0, P1, P2, c.tcw[1]);
        const float zc = gemm_row(c.Rcw, 2, P0, P1, P2, c.tcw[2]);
        const float invzc = (float)__ddiv_rn(1.0, (double)zc);
        if (!(invzc < 0)) {
            const float u = __fadd_rn(__fmul_rn(__fmul_rn(c.fx, xc), invzc), c.cx);
            const float v = __fadd_rn(__fmul_rn(__fmul_rn(c.fy, yc), invzc), c.cy);
            if (!(isfinite(u) && isfinite(v))) flags = 2;
            else if (!(u < a.minX || u > a.maxX) && !(v < a.minY || v > a.maxY)) {
                if (lp.octave < 0 || lp.octave >= a.nLevels) flags = 4;
                else {
                    q.u = u; q.v = v; q.invz = invzc;
                    flags = 1;
                }
            }
        }
    }
    a.query[p] = q;
    a.projected[p] = (uint8_t)(flags & 1);
    a.flags[p] = (uint8_t)flags;
}

// what the search reads of one projected point
struct MotionQuery {
    float u, v, ur, r;  // r: the window's radius
    int lo, hi;         // the level window
    Desc d;
};
__device__ __forceinline__ MotionQuery load_motion_query(const MotionArgs &a, const MotionFrame &fr, int p)
{
    const amos_proj_query &q = a.query[p];
    MotionQuery o;
    o.u = q.u; o.v = q.v;
    o.ur = __fsub_rn(q.u, __fmul_rn(fr.cam.mbf, q.invz));  // :1665
    const int octave = q.octave;                           // inside the table: k_motion_project
    o.r = __fmul_rn(a.pass == 2 ? fr.cam.th_retry : fr.cam.th, a.scale[octave]);
    // GetFeaturesInArea(u, v, r, minLevel, maxLevel) checks levels when minLevel > 0 || maxLevel >= 0 (Frame.cc:945): (octave, -1) when
    // bForward, (0, octave) when bBackward, else (octave - 1, octave + 1)
    if (fr.flags & 1) { o.lo = octave > 0 ? octave : INT_MIN; o.hi = INT_MAX; }
    else if (fr.flags & 2) { o.lo = 0; o.hi = octave; }
    else { o.lo = octave - 1; o.hi = octave + 1; }
    o.d = load_desc_words(q.desc);
    return o;
}

// one candidate of a window (CSR position j): its key dist << 16 | j, or none when a gate rejects it.  The occupancy test is the caller's.
__device__ __forceinline__ bool motion_candidate(const MotionQuery &q, const amos_keypoint *tk, const uint8_t *td, const float *tr, int idx, int j,
                                                 unsigned &key)
{
    const amos_keypoint k = tk[idx];
    if (k.octave < q.lo || k.octave > q.hi) return false;
    if (!(fabsf(__fsub_rn(k.x, q.u)) < q.r && fabsf(__fsub_rn(k.y, q.v)) < q.r)) return false;
    if (tr) {
        const float tt = tr[idx];
        if (tt > 0 && fabsf(__fsub_rn(q.ur, tt)) > q.r) return false;  // :1662-1669
    }
    key = ((unsigned)hamming256(q.d, load_desc(td + (size_t)idx * 32)) << 16) | (unsigned)j;  // every distance is < 256, the loop's initial bestDist
    return true;
}

// ---- the candidate loop of ORBmatcher.cc:1629-1690 against the empty frame, built like k_local_window_best2: eight lanes per point over
// the grid columns, min-reduction of dist << 16 | CSR position (cell order x * 48 + y is the candidate order: the first candidate wins
// ties).  grid = (ceil(max points * 8 / 256), frames), block = 256.
__global__ __launch_bounds__(256) void k_motion_window_best2(const MotionArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    const MotionFrame &fr = a.frames[f];
    if (a.pass == 2 && a.stats[f].n_matches >= fr.cam.retry_below) return;  // the whole work-group: the first search stands
    const int sub = t % kWindowLanes;
    const int p = fr.off0 + t / kWindowLanes;
    const bool active = p < fr.off1 && a.projected[p] != 0 && min(a.counts[f], a.capacity) > 0;
    MotionQuery q;
    CellRange c;
    c.x0 = 0; c.x1 = -1; c.y0 = c.y1 = 0;  // idle lanes walk no column and keep the group shuffles convergent
    if (active) {
        q = load_motion_query(a, fr, p);
        c = cell_range(q.u, q.v, q.r, a.minX, a.minY, a.wInv, a.hInv);
    }
    const int *cs = a.cellStart + (size_t)f * (kGridCells + 1);
    const int *it = a.items + (size_t)f * a.capacity;
    const amos_keypoint *tk = a.kps + (size_t)f * a.capacity;
    const uint8_t *td = a.desc + (size_t)f * a.capacity * 32;
    const float *tr = a.uRight ? a.uRight + (size_t)f * a.capacity : nullptr;
    unsigned best = 0xffffffffu, second = 0xffffffffu;
    for (int ix = c.x0 + sub; ix <= c.x1; ix += kWindowLanes) {
        int b, e;
        column_items(cs, c, ix, b, e);
        for (int j = b; j < e; j++) {
            unsigned key;
            if (motion_candidate(q, tk, td, tr, it[j], j, key)) top2_push(best, second, key);
        }
    }
#pragma unroll
    for (int off = kWindowLanes / 2; off > 0; off >>= 1) {
        const unsigned ob = __shfl_xor(best, off, kWindowLanes), os = __shfl_xor(second, off, kWindowLanes);
        top2_merge(best, second, ob, os);
    }
    if (p < fr.off1 && sub == 0) {
        amos_best2 res;
        res.best_idx = best == 0xffffffffu ? -1 : it[best & 0xffffu];
        res.best_dist = best == 0xffffffffu ? 256 : (int)(best >> 16);
        res.second_idx = second == 0xffffffffu ? -1 : it[second & 0xffffu];
        res.second_dist = second == 0xffffffffu ? 256 : (int)(second >> 16);
        a.best2[p] = res;
    }
}

// ---- the sequential loop of ORBmatcher.cc:1595-1702 and the pruning of :1706-1726.  One wave per frame walks the points in list order
// with a bitmap of the taken features in LDS (empty on entry: the fill of Tracking.cc:1927 is part of the call).  A feature is taken only
// when the accepted point has observations (:1658-1660).  The prepass record decides each point: best free -> the best; best taken and
// second free -> the second (the minimum of everything but the best, and it is free); both taken -> the whole wave searches the window
// again against the bitmap.  Every accepted POINT is one histogram entry (its feature and bin are kept per point in a.accepted); after the
// loop every entry of a losing bin sets its feature to -1 and lowers the count, whoever wrote the feature last.
// Everything the branches read is wave-uniform (read from one lane, or from LDS behind a barrier), so the barriers are reached by all lanes.
__global__ __launch_bounds__(64) void k_motion_accept(const MotionArgs a)
{
    __shared__ uint32_t taken[kMotionTakenWords];
    __shared__ int hist[AMOS_HISTO_LENGTH];
    const int f = blockIdx.x, lane = threadIdx.x;
    const MotionFrame &fr = a.frames[f];
    int nFirst = 0;
    if (a.pass == 2) {
        const amos_motion_stats s1 = a.stats[f];
        if (s1.n_matches >= fr.cam.retry_below) return;  // the whole wave
        nFirst = s1.n_first;
    }
    const int cap = a.capacity;
    const int off0 = fr.off0, off1 = fr.off1;
    const bool checkOri = fr.cam.check_orientation != 0;
    const int *cs = a.cellStart + (size_t)f * (kGridCells + 1);
    const int *it = a.items + (size_t)f * cap;
    const amos_keypoint *tk = a.kps + (size_t)f * cap;
    const uint8_t *td = a.desc + (size_t)f * cap * 32;
    const float *tr = a.uRight ? a.uRight + (size_t)f * cap : nullptr;
    int *match = a.match + (size_t)f * cap;
    for (int w = lane; w < kMotionTakenWords; w += 64) taken[w] = 0;
    if (lane < AMOS_HISTO_LENGTH) hist[lane] = 0;
    for (int i = lane; i < cap; i += 64) match[i] = -1;
    __syncthreads();
    const float factor = AMOS_HISTO_LENGTH / 360.0f;
    int nProjected = 0, nMatches = 0, nResearched = 0, bad = 0;
    for (int base = off0; base < off1; base += 64) {
        const int p = base + lane;
        const bool valid = p < off1;
        const int fl = valid ? a.flags[p] : 0;
        bad |= fl & 6;
        amos_best2 rec;
        rec.best_idx = rec.second_idx = -1;
        rec.best_dist = rec.second_dist = 256;
        int hasObs = 0;
        float angle = 0.f;
        if (fl & 1) {
            rec = a.best2[p];
            hasObs = a.query[p].has_obs;
            angle = a.query[p].angle;
        }
        int acc = -1;  // this lane's point: bin << 16 | feature once it is accepted
        unsigned long long todo = __ballot((fl & 1) != 0);
        nProjected += __popcll(todo);
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1;
            int bi = __builtin_amdgcn_readlane(rec.best_idx, k), bd = __builtin_amdgcn_readlane(rec.best_dist, k);
            const int si = __builtin_amdgcn_readlane(rec.second_idx, k), sd = __builtin_amdgcn_readlane(rec.second_dist, k);
            const int ho = __builtin_amdgcn_readlane(hasObs, k);
            if (bi < 0) continue;  // no candidate in the empty frame: none now
            if ((taken[bi >> 5] >> (bi & 31)) & 1u) {
                if (si < 0) continue;  // the only candidate is taken
                if (((taken[si >> 5] >> (si & 31)) & 1u) == 0) {
                    bi = si; bd = sd;
                } else {
                    nResearched++;
                    const MotionQuery q = load_motion_query(a, fr, base + k);
                    const CellRange c = cell_range(q.u, q.v, q.r, a.minX, a.minY, a.wInv, a.hInv);
                    unsigned best, second;
                    wave_window_best2(cs, it, c, lane, [&](int idx, int j, unsigned &key) {
                        return ((taken[idx >> 5] >> (idx & 31)) & 1u) == 0 && motion_candidate(q, tk, td, tr, idx, j, key);
                    }, best, second);
                    if (best == 0xffffffffu) continue;
                    bi = it[best & 0xffffu];
                    bd = (int)(best >> 16);
                }
            }
            if (bd > AMOS_TH_HIGH) continue;
            nMatches++;
            int bin = 0;
            if (checkOri) {  // :1683-1698
                const float angleLast = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(angle), k));
                float rot = __fsub_rn(angleLast, tk[bi].angle);
                if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
                bin = (int)roundf(__fmul_rn(rot, factor));
                if (bin == AMOS_HISTO_LENGTH) bin = 0;
                bin = min(max(bin, 0), AMOS_HISTO_LENGTH - 1);  // (the reference asserts it; an angle that is not finite lands in bin 0)
            }
            if (lane == k) acc = (bin << 16) | bi;
            if (lane == 0) {
                match[bi] = base + k - off0;
                if (ho) taken[bi >> 5] |= 1u << (bi & 31);
                if (checkOri) hist[bin]++;
            }
            __syncthreads();  // the bit is visible to every lane before the next point reads the bitmap
        }
        if (valid) a.accepted[p] = acc;
    }
    __threadfence_block();
    __syncthreads();  // lane 0's writes to match and hist are over before the pruning reads and overwrites
    if (checkOri) {
        // ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1866-1908): strict comparisons, the earlier bin wins a tie
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < AMOS_HISTO_LENGTH; i++) {
            const int s = hist[i];
            if (s > max1) {
                max3 = max2; max2 = max1; max1 = s;
                ind3 = ind2; ind2 = ind1; ind1 = i;
            } else if (s > max2) {
                max3 = max2; max2 = s;
                ind3 = ind2; ind2 = i;
            } else if (s > max3) {
                max3 = s; ind3 = i;
            }
        }
        if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }
        else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) ind3 = -1;
        int pruned = 0;
        for (int base = off0; base < off1; base += 64) {
            const int p = base + lane;
            const int acc = p < off1 ? a.accepted[p] : -1;
            const int bin = acc >> 16;
            const bool lose = acc >= 0 && bin != ind1 && bin != ind2 && bin != ind3;
            if (lose) match[acc & 0xffff] = -1;  // several entries of one feature write the same value
            pruned += __popcll(__ballot(lose));
        }
        nMatches -= pruned;
    }
    const unsigned long long notFinite = __ballot((bad & 2) != 0), badOctave = __ballot((bad & 4) != 0);
    if (lane == 0) {
        amos_motion_stats s;
        s.n_projected = nProjected; s.n_matches = nMatches; s.n_first = a.pass == 2 ? nFirst : nMatches; s.pass = a.pass;
        s.n_researched = nResearched; s.flags = fr.flags; s.status = (notFinite ? 1 : 0) | (badOctave ? 2 : 0); s.pad = 0;
        a.stats[f] = s;
    }
}

}  // namespace amos

using namespace amos;

static size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

extern "C" {

int amos_match_motion_model_batch_device(amos_match *m, const amos_motion_search *s)
{
    if (!m || !s || !s->d_kps || !s->d_desc || !s->d_counts || !s->d_cell_start || !s->d_items || !s->d_points || !s->point_off || !s->cameras ||
        !s->scale_factors || !s->d_query || !s->d_projected || !s->d_match || !s->d_stats || s->n_frames < 1 || s->capacity < 1 ||
        s->capacity > 65536 || s->n_levels < 1 || s->n_levels > AMOS_MAX_LEVELS || !(s->max_x > s->min_x) || !(s->max_y > s->min_y)) {
        set_error("amos_match_motion_model_batch_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    int maxPoints = 0;
    if (s->point_off[0] < 0) { set_error("amos_match_motion_model_batch_device: point_off[0] < 0"); return AMOS_ERR_INVALID; }
    for (int f = 0; f < s->n_frames; f++) {
        if (s->point_off[f + 1] < s->point_off[f]) { set_error("amos_match_motion_model_batch_device: point_off descends at %d", f); return AMOS_ERR_INVALID; }
        maxPoints = std::max(maxPoints, s->point_off[f + 1] - s->point_off[f]);
    }
    const size_t total = (size_t)s->point_off[s->n_frames];
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t bytesFrames = align64(sizeof(MotionFrame) * (size_t)s->n_frames), bytesBest = align64(sizeof(amos_best2) * total),
                 bytesAcc = align64(sizeof(int) * total);
    const int rc = grow(&m->dLocal, &m->capLocal, bytesFrames + bytesBest + bytesAcc + align64(total));
    if (rc != AMOS_OK) return rc;
    std::vector<MotionFrame> frames((size_t)s->n_frames);
    bool retry = false;
    for (int f = 0; f < s->n_frames; f++) {
        MotionFrame &fr = frames[f];
        fr.cam = s->cameras[f];
        fr.off0 = s->point_off[f];
        fr.off1 = s->point_off[f + 1];
        // :1584-1599.  twc = -Rcw^T tcw and tlc = Rlw twc + tlw are one gemm each: double accumulation, one rounding
        const amos_motion_camera &c = fr.cam;
        float twc[3];
        for (int k = 0; k < 3; k++) twc[k] = (float)(-((double)c.Rcw[k] * c.tcw[0] + (double)c.Rcw[3 + k] * c.tcw[1] + (double)c.Rcw[6 + k] * c.tcw[2]));
        const float tlcZ = (float)((double)c.Rlw[6] * twc[0] + (double)c.Rlw[7] * twc[1] + (double)c.Rlw[8] * twc[2] + (double)c.tlw[2]);
        const bool bForward = tlcZ > c.mb && !c.mono, bBackward = -tlcZ > c.mb && !c.mono;
        fr.flags = (bForward ? 1 : 0) | (bBackward ? 2 : 0);
        retry = retry || c.retry_below > 0;
    }
    // through the handle's own pinned buffer, as the local-map search does: the previous call's copy out of it has to be over first
    if (!m->localCopied) AMOS_HIP_CHECK(hipEventCreateWithFlags(&m->localCopied, hipEventDisableTiming));
    else AMOS_HIP_CHECK(hipEventSynchronize(m->localCopied));
    if (sizeof(MotionFrame) * frames.size() > m->capHLocal) {
        if (m->hLocal) (void)hipHostFree(m->hLocal);
        m->hLocal = nullptr;
        m->capHLocal = 0;
        const size_t n = std::max<size_t>(2 * sizeof(MotionFrame) * frames.size(), 4096);
        AMOS_HIP_CHECK(hipHostMalloc((void **)&m->hLocal, n, hipHostMallocDefault));
        m->capHLocal = n;
    }
    std::memcpy(m->hLocal, frames.data(), sizeof(MotionFrame) * frames.size());
    AMOS_HIP_CHECK(hipMemcpyAsync(m->dLocal, m->hLocal, sizeof(MotionFrame) * frames.size(), hipMemcpyHostToDevice, m->stream));
    AMOS_HIP_CHECK(hipEventRecord(m->localCopied, m->stream));
    MotionArgs a;
    a.kps = s->d_kps; a.desc = s->d_desc; a.counts = s->d_counts; a.cellStart = s->d_cell_start; a.items = s->d_items; a.uRight = s->d_u_right;
    a.points = s->d_points; a.frames = (const MotionFrame *)m->dLocal;
    a.query = s->d_query; a.projected = s->d_projected; a.match = s->d_match; a.stats = s->d_stats;
    a.best2 = (amos_best2 *)(m->dLocal + bytesFrames); a.accepted = (int *)(m->dLocal + bytesFrames + bytesBest);
    a.flags = m->dLocal + bytesFrames + bytesBest + bytesAcc;
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.scale[l] = l < s->n_levels ? s->scale_factors[l] : 0.f;
    a.minX = s->min_x; a.maxX = s->max_x; a.minY = s->min_y; a.maxY = s->max_y;
    a.wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(s->max_x - s->min_x);  // Frame.cc:302-303
    a.hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(s->max_y - s->min_y);
    a.capacity = s->capacity; a.nLevels = s->n_levels;
    a.pass = 1;
    if (maxPoints > 0) hipLaunchKernelGGL(k_motion_project, dim3((maxPoints + 255) / 256, s->n_frames), dim3(256), 0, m->stream, a);
    for (int pass = 1; pass <= (retry ? 2 : 1); pass++) {
        a.pass = pass;
        if (maxPoints > 0)
            hipLaunchKernelGGL(k_motion_window_best2, dim3((maxPoints * kWindowLanes + 255) / 256, s->n_frames), dim3(256), 0, m->stream, a);
        hipLaunchKernelGGL(k_motion_accept, dim3(s->n_frames), dim3(64), 0, m->stream, a);
    }
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_motion_model(amos_match *m, const amos_keypoint *kps_un, const uint8_t *desc, const float *u_right, int n,
                            const amos_last_point *points, int n_points, const amos_motion_camera *camera, const float *scale_factors,
                            int n_levels, float min_x, float max_x, float min_y, float max_y, struct amos_proj_query *query,
                            uint8_t *projected, int32_t *match, amos_motion_stats *stats)
{
    if (!m || !camera || !scale_factors || !stats || n < 0 || n > 65536 || n_points < 0 || (n > 0 && (!kps_un || !desc || !match)) ||
        (n_points > 0 && (!points || !query || !projected)) || n_levels < 1 || n_levels > AMOS_MAX_LEVELS || !(max_x > min_x) || !(max_y > min_y)) {
        set_error("amos_match_motion_model: invalid argument");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const int cap = std::max(n, 1);
    const size_t np = (size_t)n_points, np1 = std::max<size_t>(np, 1);
    // the download part of the result buffer, then the grid
    const size_t oQuery = 0, oProj = oQuery + align64(sizeof(amos_proj_query) * np1), oMatch = oProj + align64(np1),
                 oStats = oMatch + align64(sizeof(int32_t) * (size_t)cap), oEnd = oStats + align64(sizeof(amos_motion_stats)),
                 oStart = oEnd, oItems = oStart + align64(sizeof(int32_t) * (kGridCells + 1)), oAll = oItems + align64(sizeof(int32_t) * (size_t)cap);
    int rc = stage_begin(m, (size_t)cap * (sizeof(amos_keypoint) + 32 + 4 + 4) + 64 + np1 * sizeof(amos_last_point) + oEnd);
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, oAll);
    if (rc != AMOS_OK) return rc;
    // Frame::PosInGrid (Frame.cc:1007-1030)
    const float wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(max_x - min_x);
    const float hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(max_y - min_y);
    std::vector<int32_t> cell((size_t)cap, -1);
    for (int i = 0; i < n; i++) {
        const int px = (int)roundf((kps_un[i].x - min_x) * wInv), py = (int)roundf((kps_un[i].y - min_y) * hInv);
        if (px >= 0 && px < AMOS_FRAME_GRID_COLS && py >= 0 && py < AMOS_FRAME_GRID_ROWS) cell[i] = px * AMOS_FRAME_GRID_ROWS + py;
    }
    const std::vector<uint8_t> zeros(std::max<size_t>((size_t)cap * 32, sizeof(amos_last_point)), 0);  // a frame without features still hands valid arrays down
    const int32_t count = n, off[2] = {0, n_points};
    amos_motion_search s;
    s.d_kps = stage_input<amos_keypoint>(m, n ? (const void *)kps_un : zeros.data(), sizeof(amos_keypoint) * (size_t)cap);
    s.d_desc = stage_input<uint8_t>(m, n ? desc : zeros.data(), (size_t)cap * 32);
    s.d_u_right = u_right && n ? stage_input<float>(m, u_right, sizeof(float) * (size_t)cap) : nullptr;
    const int32_t *dCell = stage_input<int32_t>(m, cell.data(), sizeof(int32_t) * (size_t)cap);
    s.d_counts = stage_input<int32_t>(m, &count, sizeof(count));
    s.d_points = stage_input<amos_last_point>(m, np ? (const void *)points : zeros.data(), sizeof(amos_last_point) * np1);
    uint8_t *out = (uint8_t *)m->dOut;
    s.d_cell_start = (int32_t *)(out + oStart);
    s.d_items = (int32_t *)(out + oItems);
    s.point_off = off; s.cameras = camera; s.scale_factors = scale_factors;
    s.d_query = (amos_proj_query *)(out + oQuery); s.d_projected = out + oProj; s.d_match = (int32_t *)(out + oMatch);
    s.d_stats = (amos_motion_stats *)(out + oStats);
    s.n_frames = 1; s.capacity = cap; s.n_levels = n_levels;
    s.min_x = min_x; s.max_x = max_x; s.min_y = min_y; s.max_y = max_y;
    rc = stage_flush(m);
    if (rc != AMOS_OK) return rc;
    rc = amos_frame_grid_build_batch_device(m, dCell, s.d_counts, 1, cap, (int32_t *)(out + oStart), (int32_t *)(out + oItems));
    if (rc != AMOS_OK) return rc;
    rc = amos_match_motion_model_batch_device(m, &s);
    if (rc != AMOS_OK) return rc;
    uint8_t *h = m->hStage + stage_take(m, oEnd);
    AMOS_HIP_CHECK(hipMemcpyAsync(h, out, oEnd, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (np) {
        std::memcpy(query, h + oQuery, sizeof(amos_proj_query) * np);
        std::memcpy(projected, h + oProj, np);
    }
    if (n) std::memcpy(match, h + oMatch, sizeof(int32_t) * (size_t)n);
    std::memcpy(stats, h + oStats, sizeof(amos_motion_stats));
    return AMOS_OK;
}

}  // extern "C"
