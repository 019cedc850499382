// amos_local.hip -- step 2 of Tracking::SearchLocalPoints (Tracking.cc:2352-2389) for a batch of resident frames: Frame::isInFrustum
// (Frame.cc:761-891) with MapPoint::PredictScale (MapPoint.cc:571-586) on every local map point, then
// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (ORBmatcher.cc:70-175) over the points in view.
//
// Three launches on the matcher's stream: k_local_frustum (one thread per point), k_local_window_best2 (eight lanes per point in view:
// the best two features of its window as the frame stands on entry) and k_local_accept (one wave per frame: the reference's sequential
// greedy loop over those records).  The arithmetic is defined in include/amos_frontend.h, "local map search".
#include "amos_common.h"
#include "amos_match_core.h"
#include "amos_scene_flow.h"  // gemm_row

#include "../../include/amos_host_types.h"  // amos_map_query

#include <cmath>
#include <vector>

namespace amos {

static_assert(sizeof(amos_map_point) == 80, "amos_map_point is 80 bytes (include/amos_frontend.h)");
static_assert(sizeof(amos_local_camera) == 92, "amos_local_camera is 92 bytes");
static_assert(sizeof(amos_map_query) == 56, "amos_map_query is 56 bytes");

struct LocalFrame {
    amos_local_camera cam;
    int off0, off1;  // the frame's points
};

struct LocalArgs {
    const amos_keypoint *kps;
    const uint8_t *desc;
    const int *counts, *cellStart, *items;
    const float *uRight;
    const amos_map_point *points;
    const LocalFrame *frames;
    const uint8_t *occupied;
    amos_map_query *query;
    uint8_t *inView;
    int *match;
    amos_local_stats *stats;
    amos_best2 *best2;  // scratch, one per point
    uint8_t *flags;     // scratch, one per point: bit 0 in view, bit 1 a projection that is not finite
    float scale[AMOS_MAX_LEVELS];
    float minX, maxX, minY, maxY, wInv, hInv;
    int capacity, nLevels;
};

constexpr int kMaxTakenWords = 65536 / 32;

// ---- Frame::isInFrustum + MapPoint::PredictScale.  grid = (ceil(max points of a frame / 256), frames), block = 256.
__global__ __launch_bounds__(256) void k_local_frustum(const LocalArgs a)
{
    const LocalFrame &fr = a.frames[blockIdx.y];
    const int p = fr.off0 + blockIdx.x * 256 + threadIdx.x;
    if (p >= fr.off1) return;
    const amos_local_camera &c = fr.cam;
    const amos_map_point &mp = a.points[p];
    amos_map_query q;
    q.proj_x = q.proj_y = q.proj_xr = q.view_cos = 0.f;
    q.level = 0;
    q.has_obs = (mp.flags & AMOS_MAP_POINT_HAS_OBS) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 8; k++) reinterpret_cast<uint32_t *>(q.desc)[k] = reinterpret_cast<const uint32_t *>(mp.desc)[k];
    int flags = 0;
    if (!(mp.flags & AMOS_MAP_POINT_SKIP)) {
        const float P0 = mp.pos[0], P1 = mp.pos[1], P2 = mp.pos[2];
        const float PcX = gemm_row(c.Rcw, 0, P0, P1, P2, c.tcw[0]);
        const float PcY = gemm_row(c.Rcw, 1, P0, P1, P2, c.tcw[1]);
        const float PcZ = gemm_row(c.Rcw, 2, P0, P1, P2, c.tcw[2]);
        if (!(PcZ < 0.0f)) {
            const float invz = __fdiv_rn(1.0f, PcZ);
            const float u = __fadd_rn(__fmul_rn(__fmul_rn(c.fx, PcX), invz), c.cx);
            const float v = __fadd_rn(__fmul_rn(__fmul_rn(c.fy, PcY), invz), c.cy);
            if (!(isfinite(u) && isfinite(v))) flags = 2;
            else if (!(u < a.minX || u > a.maxX) && !(v < a.minY || v > a.maxY)) {
                const float PO0 = __fsub_rn(P0, c.Ow[0]), PO1 = __fsub_rn(P1, c.Ow[1]), PO2 = __fsub_rn(P2, c.Ow[2]);
                const double n2 = __dadd_rn(__dadd_rn(__dmul_rn((double)PO0, (double)PO0), __dmul_rn((double)PO1, (double)PO1)),
                                            __dmul_rn((double)PO2, (double)PO2));
                const float dist = (float)__dsqrt_rn(n2);
                if (!(dist < __fmul_rn(0.8f, mp.min_distance) || dist > __fmul_rn(1.2f, mp.max_distance))) {
                    const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)PO0, (double)mp.normal[0]), __dmul_rn((double)PO1, (double)mp.normal[1])),
                                                 __dmul_rn((double)PO2, (double)mp.normal[2]));
                    const float viewCos = (float)__ddiv_rn(dot, (double)dist);
                    if (!(viewCos < c.view_cos_limit)) {
                        const float ratio = __fdiv_rn(mp.max_distance, dist);
                        int level = 0;
                        for (int m = 0; m < a.nLevels; m++) level += ratio > a.scale[m] ? 1 : 0;
                        q.proj_x = u; q.proj_y = v;
                        q.proj_xr = __fsub_rn(u, __fmul_rn(c.mbf, invz));
                        q.view_cos = viewCos;
                        q.level = min(level, a.nLevels - 1);
                        flags = 1;
                    }
                }
            }
        }
    }
    a.query[p] = q;
    a.inView[p] = (uint8_t)(flags & 1);
    a.flags[p] = (uint8_t)flags;
}

// what the search reads of one point in view
struct LocalQuery {
    float u, v, ur, r;  // r: the window's radius
    int level;
    Desc d;
};
__device__ __forceinline__ LocalQuery load_local_query(const LocalArgs &a, const amos_local_camera &c, int p)
{
    const amos_map_query &q = a.query[p];
    LocalQuery o;
    o.u = q.proj_x; o.v = q.proj_y; o.ur = q.proj_xr;
    o.level = q.level;
    float r = (double)q.view_cos > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos, ORBmatcher.cc:178-184: a comparison in double
    if (c.th != 1.0f) r = __fmul_rn(r, c.th);
    o.r = __fmul_rn(r, a.scale[o.level]);
    o.d = load_desc_words(q.desc);
    return o;
}

// one candidate of a window (CSR position j): its key dist << 16 | j, or none when a gate rejects it.  The occupancy test is the caller's.
__device__ __forceinline__ bool local_candidate(const LocalQuery &q, const amos_keypoint *tk, const uint8_t *td, const float *tr, int idx, int j,
                                                unsigned &key)
{
    const amos_keypoint k = tk[idx];
    if (k.octave < q.level - 1 || k.octave > q.level) return false;  // bCheckLevels holds: maxLevel = level >= 0 (Frame.cc:945)
    if (!(fabsf(__fsub_rn(k.x, q.u)) < q.r && fabsf(__fsub_rn(k.y, q.v)) < q.r)) return false;
    if (tr) {
        const float tt = tr[idx];
        if (tt > 0 && fabsf(__fsub_rn(q.ur, tt)) > q.r) return false;
    }
    key = ((unsigned)hamming256(q.d, load_desc(td + (size_t)idx * 32)) << 16) | (unsigned)j;  // every distance is < 256, the loop's initial bestDist
    return true;
}

// ---- the window search of ORBmatcher.cc:93-160 against the frame as it stands on entry, built like k_window_best2: eight lanes per point
// over the grid columns, min-reduction of dist << 16 | CSR position.  grid = (ceil(max points * 8 / 256), frames), block = 256.
__global__ __launch_bounds__(256) void k_local_window_best2(const LocalArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    const int sub = t % kWindowLanes;
    const LocalFrame &fr = a.frames[f];
    const int p = fr.off0 + t / kWindowLanes;
    const bool active = p < fr.off1 && a.inView[p] != 0 && min(a.counts[f], a.capacity) > 0;
    LocalQuery q;
    CellRange c;
    c.x0 = 0; c.x1 = -1; c.y0 = c.y1 = 0;  // idle lanes walk no column and keep the group shuffles convergent
    if (active) {
        q = load_local_query(a, fr.cam, p);
        c = cell_range(q.u, q.v, q.r, a.minX, a.minY, a.wInv, a.hInv);
    }
    const int *cs = a.cellStart + (size_t)f * (kGridCells + 1);
    const int *it = a.items + (size_t)f * a.capacity;
    const amos_keypoint *tk = a.kps + (size_t)f * a.capacity;
    const uint8_t *td = a.desc + (size_t)f * a.capacity * 32;
    const float *tr = a.uRight ? a.uRight + (size_t)f * a.capacity : nullptr;
    const uint8_t *occ = a.occupied + (size_t)f * a.capacity;
    unsigned best = 0xffffffffu, second = 0xffffffffu;
    for (int ix = c.x0 + sub; ix <= c.x1; ix += kWindowLanes) {
        int b, e;
        column_items(cs, c, ix, b, e);
        for (int j = b; j < e; j++) {
            const int idx = it[j];
            unsigned key;
            if (occ[idx] == 0 && local_candidate(q, tk, td, tr, idx, j, key)) top2_push(best, second, key);
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

// ---- the greedy loop of ORBmatcher.cc:77-172.  One wave per frame walks the points in list order with a bitmap of the taken features
// in LDS (on entry: d_occupied).  A point whose two best features are both still free keeps its record: removing OTHER candidates
// cannot change the top two.  Otherwise the whole wave searches the point's window again against the bitmap, the lanes striding over the items of its columns.
// Everything the branches read is wave-uniform (read from one lane), so the barriers are reached by all lanes.
__global__ __launch_bounds__(64) void k_local_accept(const LocalArgs a)
{
    __shared__ uint32_t taken[kMaxTakenWords];
    const int f = blockIdx.x, lane = threadIdx.x;
    const LocalFrame &fr = a.frames[f];
    const int cap = a.capacity;
    const int off0 = fr.off0, off1 = fr.off1;
    const float nnRatio = fr.cam.nn_ratio;
    const int *cs = a.cellStart + (size_t)f * (kGridCells + 1);
    const int *it = a.items + (size_t)f * cap;
    const amos_keypoint *tk = a.kps + (size_t)f * cap;
    const uint8_t *td = a.desc + (size_t)f * cap * 32;
    const float *tr = a.uRight ? a.uRight + (size_t)f * cap : nullptr;
    const uint8_t *occ = a.occupied + (size_t)f * cap;
    int *match = a.match + (size_t)f * cap;
    for (int base = 0; base < cap; base += 64) {  // base / 32 + 1 < kMaxTakenWords: cap <= 65536
        const int i = base + lane;
        const unsigned long long m = __ballot(i < cap && occ[i] != 0);
        if (lane == 0) {
            taken[base >> 5] = (uint32_t)m;
            taken[(base >> 5) + 1] = (uint32_t)(m >> 32);
        }
        if (i < cap) match[i] = -1;
    }
    __syncthreads();
    int nInView = 0, nMatches = 0, nResearched = 0, bad = 0;
    for (int base = off0; base < off1; base += 64) {
        const int p = base + lane;
        const bool valid = p < off1;
        const int fl = valid ? a.flags[p] : 0;
        bad |= fl & 2;
        amos_best2 rec;
        rec.best_idx = rec.second_idx = -1;
        rec.best_dist = rec.second_dist = 256;
        int hasObs = 0;
        if (fl & 1) {
            rec = a.best2[p];
            hasObs = a.query[p].has_obs;
        }
        unsigned long long todo = __ballot((fl & 1) != 0);
        nInView += __popcll(todo);
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1;
            int bi = __builtin_amdgcn_readlane(rec.best_idx, k), bd = __builtin_amdgcn_readlane(rec.best_dist, k);
            int si = __builtin_amdgcn_readlane(rec.second_idx, k), sd = __builtin_amdgcn_readlane(rec.second_dist, k);
            const int ho = __builtin_amdgcn_readlane(hasObs, k);
            if (bi < 0) continue;  // no candidate on entry: none now
            const bool bt = (taken[bi >> 5] >> (bi & 31)) & 1u;
            const bool st = si >= 0 && ((taken[si >> 5] >> (si & 31)) & 1u);
            if (bt || st) {
                nResearched++;
                const LocalQuery q = load_local_query(a, fr.cam, base + k);
                const CellRange c = cell_range(q.u, q.v, q.r, a.minX, a.minY, a.wInv, a.hInv);
                unsigned best, second;
                wave_window_best2(cs, it, c, lane, [&](int idx, int j, unsigned &key) {
                    return ((taken[idx >> 5] >> (idx & 31)) & 1u) == 0 && local_candidate(q, tk, td, tr, idx, j, key);
                }, best, second);
                bi = best == 0xffffffffu ? -1 : it[best & 0xffffu];
                bd = best == 0xffffffffu ? 256 : (int)(best >> 16);
                si = second == 0xffffffffu ? -1 : it[second & 0xffffu];
                sd = second == 0xffffffffu ? 256 : (int)(second >> 16);
            }
            if (bi < 0 || bd > AMOS_TH_HIGH) continue;
            const int bestLevel = tk[bi].octave, bestLevel2 = si >= 0 ? tk[si].octave : -1;
            if (bestLevel == bestLevel2 && (float)bd > __fmul_rn(nnRatio, (float)sd)) continue;
            nMatches++;
            if (lane == 0) {
                match[bi] = base + k - off0;
                if (ho) taken[bi >> 5] |= 1u << (bi & 31);
            }
            __syncthreads();  // the bit is visible to every lane before the next point reads the bitmap
        }
    }
    const unsigned long long anyBad = __ballot(bad != 0);
    if (lane == 0) {
        amos_local_stats s;
        s.n_in_view = nInView; s.n_matches = nMatches; s.n_researched = nResearched; s.status = anyBad ? 1 : 0;
        a.stats[f] = s;
    }
}

}  // namespace amos

using namespace amos;

static size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

extern "C" {

int amos_match_local_points_batch_device(amos_match *m, const amos_local_search *s)
{
    if (!m || !s || !s->d_kps || !s->d_desc || !s->d_counts || !s->d_cell_start || !s->d_items || !s->d_points || !s->point_off || !s->cameras ||
        !s->d_occupied || !s->scale_factors || !s->d_query || !s->d_in_view || !s->d_match || !s->d_stats || s->n_frames < 1 || s->capacity < 1 ||
        s->capacity > 65536 || s->n_levels < 1 || s->n_levels > AMOS_MAX_LEVELS || !(s->max_x > s->min_x) || !(s->max_y > s->min_y)) {
        set_error("amos_match_local_points_batch_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    int maxPoints = 0;
    if (s->point_off[0] < 0) { set_error("amos_match_local_points_batch_device: point_off[0] < 0"); return AMOS_ERR_INVALID; }
    for (int f = 0; f < s->n_frames; f++) {
        if (s->point_off[f + 1] < s->point_off[f]) { set_error("amos_match_local_points_batch_device: point_off descends at %d", f); return AMOS_ERR_INVALID; }
        maxPoints = std::max(maxPoints, s->point_off[f + 1] - s->point_off[f]);
    }
    const size_t total = (size_t)s->point_off[s->n_frames];
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t bytesFrames = align64(sizeof(LocalFrame) * (size_t)s->n_frames), bytesBest = align64(sizeof(amos_best2) * total);
    const int rc = grow(&m->dLocal, &m->capLocal, bytesFrames + bytesBest + align64(total));
    if (rc != AMOS_OK) return rc;
    std::vector<LocalFrame> frames((size_t)s->n_frames);
    for (int f = 0; f < s->n_frames; f++) {
        frames[f].cam = s->cameras[f];
        frames[f].off0 = s->point_off[f];
        frames[f].off1 = s->point_off[f + 1];
    }
    // through the handle's own pinned buffer: the previous call's copy out of it has to be over before it is written again (an event,
    // not a stream synchronisation: the kernels behind that copy are not waited for)
    if (!m->localCopied) AMOS_HIP_CHECK(hipEventCreateWithFlags(&m->localCopied, hipEventDisableTiming));
    else AMOS_HIP_CHECK(hipEventSynchronize(m->localCopied));
    if (sizeof(LocalFrame) * frames.size() > m->capHLocal) {
        if (m->hLocal) (void)hipHostFree(m->hLocal);
        m->hLocal = nullptr;
        m->capHLocal = 0;
        const size_t n = std::max<size_t>(2 * sizeof(LocalFrame) * frames.size(), 4096);
        AMOS_HIP_CHECK(hipHostMalloc((void **)&m->hLocal, n, hipHostMallocDefault));
        m->capHLocal = n;
    }
    std::memcpy(m->hLocal, frames.data(), sizeof(LocalFrame) * frames.size());
    AMOS_HIP_CHECK(hipMemcpyAsync(m->dLocal, m->hLocal, sizeof(LocalFrame) * frames.size(), hipMemcpyHostToDevice, m->stream));
    AMOS_HIP_CHECK(hipEventRecord(m->localCopied, m->stream));
    LocalArgs a;
    a.kps = s->d_kps; a.desc = s->d_desc; a.counts = s->d_counts; a.cellStart = s->d_cell_start; a.items = s->d_items; a.uRight = s->d_u_right;
    a.points = s->d_points; a.frames = (const LocalFrame *)m->dLocal; a.occupied = s->d_occupied;
    a.query = s->d_query; a.inView = s->d_in_view; a.match = s->d_match; a.stats = s->d_stats;
    a.best2 = (amos_best2 *)(m->dLocal + bytesFrames); a.flags = m->dLocal + bytesFrames + bytesBest;
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.scale[l] = l < s->n_levels ? s->scale_factors[l] : 0.f;
    a.minX = s->min_x; a.maxX = s->max_x; a.minY = s->min_y; a.maxY = s->max_y;
    a.wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(s->max_x - s->min_x);  // Frame.cc:302-303
    a.hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(s->max_y - s->min_y);
    a.capacity = s->capacity; a.nLevels = s->n_levels;
    if (maxPoints > 0) {
        hipLaunchKernelGGL(k_local_frustum, dim3((maxPoints + 255) / 256, s->n_frames), dim3(256), 0, m->stream, a);
        hipLaunchKernelGGL(k_local_window_best2, dim3((maxPoints * kWindowLanes + 255) / 256, s->n_frames), dim3(256), 0, m->stream, a);
    }
    hipLaunchKernelGGL(k_local_accept, dim3(s->n_frames), dim3(64), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_local_points(amos_match *m, const amos_keypoint *kps_un, const uint8_t *desc, const float *u_right, int n,
                            const amos_map_point *points, int n_points, const amos_local_camera *camera, const uint8_t *occupied,
                            const float *scale_factors, int n_levels, float min_x, float max_x, float min_y, float max_y,
                            struct amos_map_query *query, uint8_t *in_view, int32_t *match, amos_local_stats *stats)
{
    if (!m || !camera || !scale_factors || !stats || n < 0 || n > 65536 || n_points < 0 || (n > 0 && (!kps_un || !desc || !occupied || !match)) ||
        (n_points > 0 && (!points || !query || !in_view)) || n_levels < 1 || n_levels > AMOS_MAX_LEVELS || !(max_x > min_x) || !(max_y > min_y)) {
        set_error("amos_match_local_points: invalid argument");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const int cap = std::max(n, 1);
    const size_t np = (size_t)n_points, np1 = std::max<size_t>(np, 1);
    // the download part of the result buffer, then the grid
    const size_t oQuery = 0, oInView = oQuery + align64(sizeof(amos_map_query) * np1), oMatch = oInView + align64(np1),
                 oStats = oMatch + align64(sizeof(int32_t) * (size_t)cap), oEnd = oStats + align64(sizeof(amos_local_stats)),
                 oStart = oEnd, oItems = oStart + align64(sizeof(int32_t) * (kGridCells + 1)), oAll = oItems + align64(sizeof(int32_t) * (size_t)cap);
    int rc = stage_begin(m, (size_t)cap * (sizeof(amos_keypoint) + 32 + 4 + 4 + 1) + 64 + np1 * sizeof(amos_map_point) + oEnd);
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
    const std::vector<uint8_t> zeros((size_t)cap * 32, 0);  // a frame without features still hands valid arrays down
    const int32_t count = n, off[2] = {0, n_points};
    amos_local_search s;
    s.d_kps = stage_input<amos_keypoint>(m, n ? (const void *)kps_un : zeros.data(), sizeof(amos_keypoint) * (size_t)cap);
    s.d_desc = stage_input<uint8_t>(m, n ? desc : zeros.data(), (size_t)cap * 32);
    s.d_u_right = u_right && n ? stage_input<float>(m, u_right, sizeof(float) * (size_t)cap) : nullptr;
    const int32_t *dCell = stage_input<int32_t>(m, cell.data(), sizeof(int32_t) * (size_t)cap);
    s.d_counts = stage_input<int32_t>(m, &count, sizeof(count));
    s.d_occupied = stage_input<uint8_t>(m, n ? occupied : zeros.data(), (size_t)cap);
    s.d_points = stage_input<amos_map_point>(m, np ? (const void *)points : zeros.data(), np ? sizeof(amos_map_point) * np : 16);
    uint8_t *out = (uint8_t *)m->dOut;
    s.d_cell_start = (int32_t *)(out + oStart);
    s.d_items = (int32_t *)(out + oItems);
    s.point_off = off; s.cameras = camera; s.scale_factors = scale_factors;
    s.d_query = (amos_map_query *)(out + oQuery); s.d_in_view = out + oInView; s.d_match = (int32_t *)(out + oMatch);
    s.d_stats = (amos_local_stats *)(out + oStats);
    s.n_frames = 1; s.capacity = cap; s.n_levels = n_levels;
    s.min_x = min_x; s.max_x = max_x; s.min_y = min_y; s.max_y = max_y;
    rc = stage_flush(m);
    if (rc != AMOS_OK) return rc;
    rc = amos_frame_grid_build_batch_device(m, dCell, s.d_counts, 1, cap, (int32_t *)(out + oStart), (int32_t *)(out + oItems));
    if (rc != AMOS_OK) return rc;
    rc = amos_match_local_points_batch_device(m, &s);
    if (rc != AMOS_OK) return rc;
    uint8_t *h = m->hStage + stage_take(m, oEnd);
    AMOS_HIP_CHECK(hipMemcpyAsync(h, out, oEnd, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (np) {
        std::memcpy(query, h + oQuery, sizeof(amos_map_query) * np);
        std::memcpy(in_view, h + oInView, np);
    }
    if (n) std::memcpy(match, h + oMatch, sizeof(int32_t) * (size_t)n);
    std::memcpy(stats, h + oStats, sizeof(amos_local_stats));
    return AMOS_OK;
}

}  // extern "C"
