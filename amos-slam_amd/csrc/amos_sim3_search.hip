// amos_sim3_search.hip -- step 3 of LoopClosing::ComputeSim3's candidate loop (LoopClosing.cc:454): ORBmatcher::SearchBySim3
// (ORBmatcher.cc:1314-1555) for a batch of pairs (keyframe-1 slot, keyframe-2 slot) of resident keyframes, reading the Sim3Solver's
// result records and rows (amos_sim3.hip) in place.  The arithmetic is amos_sim3_search_core.h, defined in include/amos_frontend.h,
// "loop-closing Sim3 search"; tests/sim3_search_restatement.py is the same in Python and the GPU tests hold the kernels to it with ==.
//
// TWO launches on the matcher's stream, eight lanes per source feature (the AMOS_FUSE_SIM3 search of k_fuse behind another projection):
//   k_sim3_search_12  copies the row, marks vbAlreadyMatched2 in a byte plane of the call's scratch (zeroed ahead of the launch; several
//                     features may store the same 1 to one byte), projects KF1's free points into KF2 and writes vnMatch1
//   k_sim3_search_21  projects KF2's unmarked points into KF1, writes vnMatch2, and the group's first lane does the agreement from KF2's
//                     side: with i1 = vnMatch2[i2] >= 0, vnMatch1[i1] == i2 writes d_match_out[i1] = i2.  That is the set the reference's
//                     loop over i1 accepts; vnMatch1 is single-valued, so each i1 is written at most once, and i1 was free, so the only
//                     other writer of that entry is the copy one launch earlier.
// Direction 2 reads what direction 1 marked and the agreement reads all of vnMatch1: that is the launch boundary.  One work-group per pair
// would need no boundary, but the usual call has one to three pairs and would occupy as many CUs.
// A skipped pair, or one with a slot outside the frames, is recognised alike in both kernels (from the record the call uploaded, or the
// solver's result row): its blocks write nothing but the stats record (block 0 of k_sim3_search_12).
#include "amos_common.h"
#include "amos_projection_search.h"
#include "amos_sim3_search_core.h"

#include "../../include/amos_host_types.h"  // amos_frame_view

#include <cmath>
#include <vector>

namespace amos {

static_assert(sizeof(amos_sim3_search_pair) == 60, "amos_sim3_search_pair is 60 bytes (include/amos_frontend.h)");
static_assert(sizeof(amos_sim3_search_stats) == 32, "amos_sim3_search_stats is 32 bytes");
static_assert(sizeof(amos_map_point) == 80 && sizeof(amos_sim3_camera) == 64, "amos_map_point is 80 bytes, amos_sim3_camera 64");
static_assert(offsetof(amos_sim3_result, t12) == 36 && offsetof(amos_sim3_result, s12) == 48, "R12, t12, s12 are the result's first 13 floats");

struct S3SearchArgs : ProjArgs {
    const amos_map_point *points;            // [frames][capacity]
    const amos_sim3_camera *cameras;         // [frames], uploaded by the call
    const amos_sim3_search_pair *pairs;      // [pairs], uploaded by the call
    const amos_sim3_result *sim3;            // [pairs] or null
    const int *pairs1, *pairs2;
    const int *matchIn;                      // [pairs][capacity]
    int *matchOut, *match1, *match2;         // [pairs][capacity]
    uint8_t *matched2;                       // [pairs][capacity]: vbAlreadyMatched2, zeroed in front of the launches
    amos_sim3_search_stats *stats;           // zeroed in front of the launches
    int nFrames;
};

struct S3SearchPair {
    int f1, f2, n1, n2;
    float th;
    sim3::SearchHops h;
};

// -> 0: the pair runs; 1: skipped; -4: a slot outside the frames.  Block-uniform.
__device__ __forceinline__ int search_pair(const S3SearchArgs &a, int p, S3SearchPair &s)
{
    const amos_sim3_search_pair &pr = a.pairs[p];
    s.f1 = a.pairs1[p]; s.f2 = a.pairs2[p];
    if (s.f1 < 0 || s.f1 >= a.nFrames || s.f2 < 0 || s.f2 >= a.nFrames) return -4;
    if (!pr.enabled) return 1;
    const float *R = pr.R12, *t = pr.t12;
    float sc = pr.s12;
    if (a.sim3) {
        const amos_sim3_result &r = a.sim3[p];
        if (!r.has_sim3 || r.code != 0) return 1;
        R = r.R12; t = r.t12; sc = r.s12;
    }
    s.n1 = min(max(a.counts[s.f1], 0), a.capacity);
    s.n2 = min(max(a.counts[s.f2], 0), a.capacity);
    s.th = pr.th;
    sim3::sim3_search_hops(R, t, sc, s.h);
    return 0;
}

// One direction for the lanes of a group: feature i of keyframe `from` (source: it has a point to project and is free on its side) through
// (Rfw, tfw) and the hop into keyframe `into`, KF1's intrinsics K -> the accepted feature of `into` or -1; inView: its window was searched.
// All lanes of a group call it.
__device__ __forceinline__ int search_direction(const S3SearchArgs &a, bool source, int from, int into, int nInto, int i, int sub, const float *hopR,
                                                const float *hopT, const float *K, float th, bool &inView)
{
    WindowQuery q;
    q.u = q.v = q.ur = q.r = 0.f;
    q.lo = q.hi = 0;
    inView = false;
    if (source) {
        const amos_map_point *mp = a.points + (size_t)from * a.capacity + i;
        if (!(mp->flags & AMOS_MAP_POINT_SKIP)) {
            const amos_sim3_camera &cf = a.cameras[from];
            sim3::SearchProjection pr;
            if (sim3::sim3_search_project(cf.Rcw, cf.tcw, hopR, hopT, K, mp->pos, mp->min_distance, mp->max_distance, a.scale, a.nLevels, a.minX,
                                          a.maxX, a.minY, a.maxY, pr) == 0) {
                q.u = pr.u; q.v = pr.v;
                q.lo = pr.level - 1; q.hi = pr.level;
                q.r = __fmul_rn(th, a.scale[pr.level]);
                q.d = load_desc_words(mp->desc);
                inView = true;
            }
        }
    }
    FrameView fv = frame_view(a, into);
    fv.tr = nullptr;  // no right-coordinate gate
    unsigned best, second;
    lanes_window_keys(a, fv, q, inView && nInto > 0, sub, kInitDist, [](int) { return true; }, best, second);
    if (best == 0xffffffffu || (int)(best >> 16) > AMOS_TH_HIGH) return -1;
    return fv.it[best & 0xffffu];
}

// ---- grid = (ceil(capacity * 8 / 256), pairs), block = 256.  No lane leaves before the group shuffles; the early return is per block.
__global__ __launch_bounds__(256) void k_sim3_search_12(const S3SearchArgs a)
{
    const int p = blockIdx.y;
    S3SearchPair s;
    const int why = search_pair(a, p, s);
    if (why != 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (why == 1) a.stats[p].skipped = 1;
            else a.stats[p].code = why;
        }
        return;
    }
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i1 = t / kWindowLanes, sub = t % kWindowLanes;
    const bool inRow = i1 < a.capacity, lead = inRow && sub == 0;
    const size_t row = (size_t)p * a.capacity, o = row + (inRow ? i1 : 0);
    const int e = inRow ? a.matchIn[o] : 0;
    if (lead && a.matchOut != a.matchIn) a.matchOut[o] = e;
    if (lead && i1 < s.n1 && e >= 0 && e < s.n2) a.matched2[row + e] = 1;
    bool inView;
    const amos_sim3_camera &c1 = a.cameras[s.f1];
    const int got = search_direction(a, i1 < s.n1 && e == -1, s.f1, s.f2, s.n2, i1, sub, s.h.sR21, s.h.t21, &c1.fx, s.th, inView);
    if (lead) a.match1[o] = got;
    const unsigned long long seen = __ballot(lead && inView), single = __ballot(lead && got >= 0);
    if ((threadIdx.x & 63) == 0) {
        if (seen) atomicAdd(&a.stats[p].n_in_view_12, __popcll(seen));
        if (single) atomicAdd(&a.stats[p].n_single_12, __popcll(single));
    }
}

__global__ __launch_bounds__(256) void k_sim3_search_21(const S3SearchArgs a)
{
    const int p = blockIdx.y;
    S3SearchPair s;
    if (search_pair(a, p, s) != 0) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i2 = t / kWindowLanes, sub = t % kWindowLanes;
    const bool inRow = i2 < a.capacity, lead = inRow && sub == 0;
    const size_t row = (size_t)p * a.capacity, o = row + (inRow ? i2 : 0);
    const bool source = i2 < s.n2 && !a.matched2[o];
    bool inView;
    const amos_sim3_camera &c1 = a.cameras[s.f1];
    const int got = search_direction(a, source, s.f2, s.f1, s.n1, i2, sub, s.h.sR12, s.h.t12, &c1.fx, s.th, inView);
    bool agreed = false;
    if (lead) {
        a.match2[o] = got;
        if (got >= 0 && a.match1[row + got] == i2) {  // :1539-1552 from KF2's side
            a.matchOut[row + got] = i2;
            agreed = true;
        }
    }
    const unsigned long long seen = __ballot(lead && inView), single = __ballot(lead && got >= 0), found = __ballot(agreed);
    if ((threadIdx.x & 63) == 0) {
        if (seen) atomicAdd(&a.stats[p].n_in_view_21, __popcll(seen));
        if (single) atomicAdd(&a.stats[p].n_single_21, __popcll(single));
        if (found) atomicAdd(&a.stats[p].n_found, __popcll(found));
    }
}

}  // namespace amos

using namespace amos;

static bool s3s_camera_ok(const char *name, const amos_sim3_camera &c, int k)
{
    bool ok = std::isfinite(c.fx) && std::isfinite(c.fy) && std::isfinite(c.cx) && std::isfinite(c.cy);
    for (int i = 0; i < 9; i++) ok = ok && std::isfinite(c.Rcw[i]);
    for (int i = 0; i < 3; i++) ok = ok && std::isfinite(c.tcw[i]);
    if (!ok) set_error("%s: camera %d is not finite", name, k);
    return ok;
}

// an enabled pair's record: th, and the Sim3 when the host supplies it
static bool s3s_pair_ok(const char *name, const amos_sim3_search_pair &p, bool hostSim3, int k)
{
    if (!p.enabled) return true;
    if (!(std::isfinite(p.th) && p.th > 0.f)) { set_error("%s: pair %d: th is not finite or <= 0", name, k); return false; }
    if (!hostSim3) return true;
    bool ok = std::isfinite(p.s12) && p.s12 > 0.f;
    for (int i = 0; i < 9; i++) ok = ok && std::isfinite(p.R12[i]);
    for (int i = 0; i < 3; i++) ok = ok && std::isfinite(p.t12[i]);
    if (!ok) set_error("%s: pair %d: the Sim3 is not finite or has s12 <= 0", name, k);
    return ok;
}

extern "C" {

int amos_match_sim3_search_batch_device(amos_match *m, const amos_sim3_search *s)
{
    static const char *name = "amos_match_sim3_search_batch_device";
    if (!m || !s || !s->d_kps || !s->d_desc || !s->d_counts || !s->d_cell_start || !s->d_items || !s->d_points || !s->cameras || !s->scale_factors ||
        !s->d_pairs_1 || !s->d_pairs_2 || !s->pairs || !s->d_match12 || !s->d_match_out || !s->d_match1 || !s->d_match2 || !s->d_stats ||
        s->n_pairs < 1 || s->n_frames < 1 || s->capacity < 1 || s->capacity > 65536 || s->n_levels < 1 || s->n_levels > AMOS_MAX_LEVELS ||
        !(s->max_x > s->min_x) || !(s->max_y > s->min_y)) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    if (s->d_match1 == s->d_match12 || s->d_match1 == s->d_match_out || s->d_match2 == s->d_match12 || s->d_match2 == s->d_match_out ||
        s->d_match1 == s->d_match2) {
        set_error("%s: d_match1 or d_match2 aliases a row array", name);
        return AMOS_ERR_INVALID;
    }
    for (int k = 0; k < s->n_frames; k++)
        if (!s3s_camera_ok(name, s->cameras[k], k)) return AMOS_ERR_INVALID;
    for (int k = 0; k < s->n_pairs; k++)
        if (!s3s_pair_ok(name, s->pairs[k], s->d_sim3 == nullptr, k)) return AMOS_ERR_INVALID;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    // the call's scratch: the pair records, the cameras, vbAlreadyMatched2
    const size_t np = (size_t)s->n_pairs, plane = np * (size_t)s->capacity;
    const size_t bytesPairs = align64(sizeof(amos_sim3_search_pair) * np), bytesCams = align64(sizeof(amos_sim3_camera) * (size_t)s->n_frames);
    int rc = grow(&m->dLocal, &m->capLocal, bytesPairs + bytesCams + align64(plane));
    if (rc != AMOS_OK) return rc;
    std::vector<uint8_t> host(bytesPairs + bytesCams, 0);
    std::memcpy(host.data(), s->pairs, sizeof(amos_sim3_search_pair) * np);
    std::memcpy(host.data() + bytesPairs, s->cameras, sizeof(amos_sim3_camera) * (size_t)s->n_frames);
    rc = upload_frames(m, host.data(), host.size());
    if (rc != AMOS_OK) return rc;
    S3SearchArgs a;
    a.kps = s->d_kps; a.desc = s->d_desc; a.counts = s->d_counts; a.cellStart = s->d_cell_start; a.items = s->d_items; a.uRight = nullptr;
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.scale[l] = l < s->n_levels ? s->scale_factors[l] : 0.f;
    a.minX = s->min_x; a.maxX = s->max_x; a.minY = s->min_y; a.maxY = s->max_y;
    a.wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(s->max_x - s->min_x);
    a.hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(s->max_y - s->min_y);
    a.capacity = s->capacity; a.nLevels = s->n_levels;
    a.points = s->d_points;
    a.pairs = (const amos_sim3_search_pair *)m->dLocal; a.cameras = (const amos_sim3_camera *)(m->dLocal + bytesPairs);
    a.sim3 = s->d_sim3; a.pairs1 = s->d_pairs_1; a.pairs2 = s->d_pairs_2;
    a.matchIn = s->d_match12; a.matchOut = s->d_match_out; a.match1 = s->d_match1; a.match2 = s->d_match2;
    a.matched2 = m->dLocal + bytesPairs + bytesCams; a.stats = s->d_stats; a.nFrames = s->n_frames;
    AMOS_HIP_CHECK(hipMemsetAsync(a.matched2, 0, plane, m->stream));
    AMOS_HIP_CHECK(hipMemsetAsync(s->d_stats, 0, sizeof(amos_sim3_search_stats) * np, m->stream));
    const dim3 grid = window_grid(s->capacity, s->n_pairs);
    hipLaunchKernelGGL(k_sim3_search_12, grid, dim3(256), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_sim3_search_21, grid, dim3(256), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_sim3_search(amos_match *m, const amos_frame_view *kf1, const amos_map_point *points1, const amos_frame_view *kf2,
                           const amos_map_point *points2, const amos_sim3_camera *cameras, const amos_sim3_search_pair *sim3,
                           const float *scale_factors, int n_levels, const int32_t *match12, int32_t *match_out, int32_t *match1,
                           int32_t *match2, amos_sim3_search_stats *stats)
{
    static const char *name = "amos_match_sim3_search";
    bool ok = m && kf1 && kf2 && cameras && sim3 && scale_factors && stats && n_levels >= 1 && n_levels <= AMOS_MAX_LEVELS;
    const amos_frame_view *kfs[2] = {kf1, kf2};
    const amos_map_point *pts[2] = {points1, points2};
    for (int k = 0; ok && k < 2; k++) {
        const amos_frame_view &v = *kfs[k];
        ok = v.n >= 0 && v.n <= 65536 && (v.n == 0 || (v.keys_un && v.descriptors && pts[k])) && v.min_x == kf1->min_x && v.max_x == kf1->max_x &&
             v.min_y == kf1->min_y && v.max_y == kf1->max_y;
    }
    ok = ok && kf1->max_x > kf1->min_x && kf1->max_y > kf1->min_y && (kf1->n == 0 || (match12 && match_out));
    if (!ok) {
        set_error("%s: invalid argument (a NULL pointer, a count or n_levels out of range, keyframes with different or empty image bounds)", name);
        return AMOS_ERR_INVALID;
    }
    if (!s3s_camera_ok(name, cameras[0], 0) || !s3s_camera_ok(name, cameras[1], 1) || !s3s_pair_ok(name, *sim3, true, 0)) return AMOS_ERR_INVALID;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const int n1 = kf1->n, n2 = kf2->n;
    const size_t cap = (size_t)std::max(std::max(n1, n2), 1);
    // the download: match_out, match1, match2 [cap], the stats; then the grids
    const size_t oM1 = align64(4 * cap), oM2 = oM1 + align64(4 * cap), oStats = oM2 + align64(4 * cap), oEnd = oStats + align64(sizeof(amos_sim3_search_stats)),
                 oItems = oEnd + align64(4 * 2 * (kGridCells + 1)), oAll = oItems + align64(4 * 2 * cap);
    int rc = stage_begin(m, 2 * cap * (sizeof(amos_keypoint) + 32 + 4 + sizeof(amos_map_point)) + 4 * cap + 64 * 10 + oEnd);
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, oAll);
    if (rc != AMOS_OK) return rc;
    // the two keyframes are slots 0 and 1 of [2][cap] arrays (an empty keyframe still hands valid arrays down), Frame::PosInGrid on the way
    const float wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(kf1->max_x - kf1->min_x);
    const float hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(kf1->max_y - kf1->min_y);
    const size_t hKps = stage_take(m, 2 * cap * sizeof(amos_keypoint)), hDesc = stage_take(m, 2 * cap * 32), hCell = stage_take(m, 2 * cap * 4),
                 hPts = stage_take(m, 2 * cap * sizeof(amos_map_point)), hRow = stage_take(m, 4 * cap), hCounts = stage_take(m, 8), hSlots = stage_take(m, 8);
    std::memset(m->hStage + hKps, 0, 2 * cap * sizeof(amos_keypoint));
    std::memset(m->hStage + hDesc, 0, 2 * cap * 32);
    int32_t *cell = (int32_t *)(m->hStage + hCell), *row = (int32_t *)(m->hStage + hRow), *counts = (int32_t *)(m->hStage + hCounts),
            *slots = (int32_t *)(m->hStage + hSlots);
    amos_map_point *hp = (amos_map_point *)(m->hStage + hPts);
    std::fill(cell, cell + 2 * cap, -1);
    std::fill(row, row + cap, -1);
    std::memset(hp, 0, 2 * cap * sizeof(amos_map_point));
    for (size_t i = 0; i < 2 * cap; i++) hp[i].flags = AMOS_MAP_POINT_SKIP;
    for (size_t k = 0; k < 2; k++) {
        const amos_frame_view &v = *kfs[k];
        counts[k] = v.n;
        if (!v.n) continue;
        std::memcpy(m->hStage + hKps + k * cap * sizeof(amos_keypoint), v.keys_un, sizeof(amos_keypoint) * (size_t)v.n);
        std::memcpy(m->hStage + hDesc + k * cap * 32, v.descriptors, 32 * (size_t)v.n);
        std::memcpy(hp + k * cap, pts[k], sizeof(amos_map_point) * (size_t)v.n);
        for (int i = 0; i < v.n; i++) cell[k * cap + i] = pos_in_grid(v.keys_un[i].x, v.keys_un[i].y, v.min_x, v.min_y, wInv, hInv);
    }
    if (n1) std::memcpy(row, match12, 4 * (size_t)n1);
    slots[0] = 0; slots[1] = 1;
    uint8_t *out = (uint8_t *)m->dOut;
    amos_sim3_search s;
    s.d_kps = (const amos_keypoint *)(m->dArena + hKps); s.d_desc = m->dArena + hDesc; s.d_counts = (const int32_t *)(m->dArena + hCounts);
    s.d_cell_start = (int32_t *)(out + oEnd); s.d_items = (int32_t *)(out + oItems);
    s.d_points = (const amos_map_point *)(m->dArena + hPts);
    s.cameras = cameras; s.scale_factors = scale_factors;
    s.d_pairs_1 = (const int32_t *)(m->dArena + hSlots); s.d_pairs_2 = s.d_pairs_1 + 1;
    s.pairs = sim3; s.d_sim3 = nullptr;
    s.d_match12 = (const int32_t *)(m->dArena + hRow);
    s.d_match_out = (int32_t *)out; s.d_match1 = (int32_t *)(out + oM1); s.d_match2 = (int32_t *)(out + oM2);
    s.d_stats = (amos_sim3_search_stats *)(out + oStats);
    s.n_frames = 2; s.n_pairs = 1; s.capacity = (int32_t)cap; s.n_levels = n_levels;
    s.min_x = kf1->min_x; s.max_x = kf1->max_x; s.min_y = kf1->min_y; s.max_y = kf1->max_y;
    if ((rc = stage_flush(m)) != AMOS_OK ||
        (rc = amos_frame_grid_build_batch_device(m, (const int32_t *)(m->dArena + hCell), s.d_counts, 2, (int)cap, (int32_t *)(out + oEnd),
                                                 (int32_t *)(out + oItems))) != AMOS_OK ||
        (rc = amos_match_sim3_search_batch_device(m, &s)) != AMOS_OK) return rc;
    const uint8_t *h = m->hStage + stage_take(m, oEnd);
    AMOS_HIP_CHECK(hipMemcpyAsync((void *)h, out, oEnd, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    std::memcpy(stats, h + oStats, sizeof(amos_sim3_search_stats));
    if (stats->skipped || stats->code != 0) return AMOS_OK;
    if (n1) {
        std::memcpy(match_out, h, 4 * (size_t)n1);
        if (match1) std::memcpy(match1, h + oM1, 4 * (size_t)n1);
    }
    if (n2 && match2) std::memcpy(match2, h + oM2, 4 * (size_t)n2);
    return AMOS_OK;
}

}  // extern "C"
