// amos_loop_points.hip -- the last step of LoopClosing::ComputeSim3 (LoopClosing.cc:534-546) for a batch of QUERIES (current keyframe slot,
// point range, Scw, row) on resident keyframes: ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:388-512)
// and nTotalMatches >= 40.  The Scw is the query record's, or row q of amos_match_sim3_optimize_batch_device's results read in place.
//
// Launches on the matcher's stream, the relocalisation search's shape (amos_reloc.hip): k_loop_found (only when a query has
// found_from_match: one thread per feature marks the point its entry match names through d_point_of_feature2), k_loop_project (one thread
// per point: Scw's decomposition and the AMOS_FUSE_SIM3 pre-filter), k_loop_window_best2 (eight lanes per point in view: the best two
// features of its window among those free on entry) and k_loop_accept (one wave per query: the reference's sequential greedy loop over
// those records).  A skipped query's work-groups return at once.  The arithmetic is defined in include/amos_frontend.h, "loop-closing point
// search".
#include "amos_common.h"
#include "amos_projection_search.h"
#include "amos_loop_points_core.h"

#include "../../include/amos_host_types.h"  // amos_frame_view

#include <vector>

namespace amos {

static_assert(sizeof(amos_loop_points_query) == 108, "amos_loop_points_query is 108 bytes (include/amos_frontend.h)");
static_assert(sizeof(amos_loop_points_stats) == 32, "amos_loop_points_stats is 32 bytes");
static_assert(sizeof(amos_map_point) == 80 && sizeof(amos_sim3_opt_result) == 256, "amos_map_point is 80 bytes, amos_sim3_opt_result 256");

struct LoopQuery {
    amos_loop_points_query q;
    int first, count;  // the query's points in d_points
    int off;           // its records in the call's scratch (queries that share a point range do not share records)
};

// what k_loop_project leaves of one point
struct LoopPoint {
    float u, v;
    int level, flags;
};
enum { kLoopInView = 1, kLoopNotFinite = 2, kLoopCandidate = 4 };

struct LoopArgs : ProjArgs {
    const amos_map_point *points;
    const LoopQuery *queries;
    const amos_sim3_opt_result *opt;  // one per query, or null
    const int *matched;               // [queries][capacity]: on entry, -1 = free
    const uint8_t *found;             // one per point of d_points, or null
    const int *pointOfFeature2;       // [queries][capacity], or null
    int *loopMatch;                   // [queries][capacity]
    amos_loop_points_stats *stats;
    LoopPoint *proj;      // scratch, one per (query, point)
    amos_best2 *best2;    // scratch, one per (query, point)
    uint8_t *foundMatch;  // scratch, one per (query, point), zeroed by the entry; null: no query asks
};

// the query runs: enabled, and with d_opt a row that carries an optimised Sim3 with enough inliers (LoopClosing.cc:464).  Block-uniform.
__device__ __forceinline__ bool loop_runs(const LoopArgs &a, int k)
{
    const amos_loop_points_query &q = a.queries[k].q;
    if (!q.enabled) return false;
    if (!a.opt) return true;
    const amos_sim3_opt_result &r = a.opt[k];
    return r.skipped == 0 && r.code == 0 && r.n_inliers >= q.min_inliers;
}

// ---- spAlreadyFound from the entry row (:407-408).  grid = (ceil(capacity / 256), queries), block = 256.
__global__ __launch_bounds__(256) void k_loop_found(const LoopArgs a)
{
    const int k = blockIdx.y;
    const LoopQuery &lq = a.queries[k];
    if (!lq.q.found_from_match || !loop_runs(a, k)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(max(a.counts[lq.q.frame], 0), a.capacity)) return;
    const int j = a.matched[(size_t)k * a.capacity + i];
    if (j < 0 || j >= a.capacity) return;
    const int p = a.pointOfFeature2[(size_t)k * a.capacity + j];
    if (p >= 0 && p < lq.count) a.foundMatch[lq.off + p] = 1;  // several features of one point write the same value
}

// ---- :397-403 and the pre-filter of :416-462.  grid = (ceil(max points of a query / 256), queries), block = 256.
__global__ __launch_bounds__(256) void k_loop_project(const LoopArgs a)
{
    const int k = blockIdx.y;
    if (!loop_runs(a, k)) return;
    const LoopQuery &lq = a.queries[k];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= lq.count) return;
    const amos_map_point &mp = a.points[lq.first + i];
    LoopPoint o;
    o.u = o.v = 0.f;
    o.level = 0;
    o.flags = 0;
    const bool found = (a.found && a.found[lq.first + i] != 0) || (a.foundMatch && lq.q.found_from_match && a.foundMatch[lq.off + i] != 0);
    if (!(mp.flags & AMOS_MAP_POINT_SKIP) && !found) {
        o.flags = kLoopCandidate;
        loop::Unscaled cw;
        loop::unscale(a.opt ? a.opt[k].Scw : lq.q.Scw, cw);
        KeyframeProjection pj;
        const int why = keyframe_prefilter(a, cw.Rcw, cw.tcw, cw.Ow, lq.q.fx, lq.q.fy, lq.q.cx, lq.q.cy, mp, pj);
        if (why == 0) {
            o.u = pj.u; o.v = pj.v; o.level = pj.level;
            o.flags |= kLoopInView;
        } else if (why == kViewImage && !(isfinite(pj.u) && isfinite(pj.v))) o.flags |= kLoopNotFinite;
    }
    a.proj[lq.off + i] = o;
}

// what the search reads of one point in view
__device__ __forceinline__ WindowQuery load_loop_query(const LoopArgs &a, const LoopQuery &lq, int i)
{
    const LoopPoint &p = a.proj[lq.off + i];
    WindowQuery o;
    o.u = p.u; o.v = p.v; o.ur = 0.f;  // no right gate
    o.r = __fmul_rn(lq.q.th, a.scale[p.level]);
    o.lo = p.level - 1; o.hi = p.level;  // :486-487
    o.d = load_desc_words(a.points[lq.first + i].desc);
    return o;
}

// ---- the candidate loop of :476-497 against the keyframe as it stands on entry: the best two of the features that are free then.
// grid = (ceil(max points * 8 / 256), queries), block = 256.
__global__ __launch_bounds__(256) void k_loop_window_best2(const LoopArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (!loop_runs(a, k)) return;  // the whole work-group
    const LoopQuery &lq = a.queries[k];
    const int i = t / kWindowLanes;
    const int count = min(max(a.counts[lq.q.frame], 0), a.capacity);
    const bool active = i < lq.count && (a.proj[lq.off + i].flags & kLoopInView) != 0 && count > 0;
    WindowQuery q;
    if (active) q = load_loop_query(a, lq, i);
    const int *onEntry = a.matched + (size_t)k * a.capacity;
    lanes_window_best2(a, frame_view(a, lq.q.frame), q, active, t % kWindowLanes, kInitDist, [&](int idx) { return onEntry[idx] == -1; },
                       i < lq.count ? a.best2 + lq.off + i : nullptr);
}

// ---- the sequential loop of :405-507 and the count of LoopClosing.cc:538-546.  One wave per query walks the points in list order with a
// bitmap of the occupied features in LDS (on entry: d_matched != -1).  Every accept sets its bit.  The prepass record decides each point:
// its best-on-entry distance above max_dist -> none (what is free now was free on entry, so nothing nearer exists); best free -> the best;
// best taken and the second above max_dist -> none (the second is the minimum of everything but the best); best taken and second free ->
// the second; both taken -> the whole wave searches the window again against the bitmap.
// Everything the branches read is wave-uniform (read from one lane, or from LDS behind a barrier), so the barriers are reached by all lanes.
__global__ __launch_bounds__(64) void k_loop_accept(const LoopArgs a)
{
    __shared__ TakenBitmap taken;
    const int k = blockIdx.x, lane = threadIdx.x;
    if (!loop_runs(a, k)) {  // the whole wave
        if (lane == 0) {
            amos_loop_points_stats s = {};
            s.skipped = 1;
            a.stats[k] = s;
        }
        return;
    }
    const LoopQuery &lq = a.queries[k];
    const int cap = a.capacity, count = min(max(a.counts[lq.q.frame], 0), cap);
    const int nPoints = lq.count, maxDist = lq.q.max_dist;
    const FrameView fv = frame_view(a, lq.q.frame);
    const int *onEntry = a.matched + (size_t)k * cap;
    int *loopMatch = a.loopMatch + (size_t)k * cap;
    int nOccupied = 0;
    for (int base = 0; base < cap; base += 64) {  // base / 32 + 1 < kTakenWords: cap <= 65536
        const int i = base + lane;
        const bool set = i < cap && onEntry[i] != -1;
        const unsigned long long m = __ballot(set);
        nOccupied += __popcll(__ballot(set && i < count));
        if (i < cap) loopMatch[i] = -1;  // (complete before the barrier below; an accept writes its entry behind it)
        if (lane == 0) {
            taken.w[base >> 5] = (uint32_t)m;
            taken.w[(base >> 5) + 1] = (uint32_t)(m >> 32);
        }
    }
    __syncthreads();
    int nCandidates = 0, nInView = 0, nMatches = 0, nResearched = 0, bad = 0;
    for (int base = 0; base < nPoints; base += 64) {
        const int i = base + lane;
        const int fl = i < nPoints ? a.proj[lq.off + i].flags : 0;
        bad |= fl & kLoopNotFinite;
        nCandidates += __popcll(__ballot((fl & kLoopCandidate) != 0));
        amos_best2 rec = best2_from_keys(0xffffffffu, 0xffffffffu, nullptr, kInitDist);  // none
        if (fl & kLoopInView) rec = a.best2[lq.off + i];
        int acc = -1;  // the feature this lane's point is accepted at
        unsigned long long todo = __ballot((fl & kLoopInView) != 0);
        nInView += __popcll(todo);
        while (todo) {
            const int j = __ffsll(todo) - 1;
            todo &= todo - 1;
            int bi = __builtin_amdgcn_readlane(rec.best_idx, j), bd = __builtin_amdgcn_readlane(rec.best_dist, j);
            const int si = __builtin_amdgcn_readlane(rec.second_idx, j), sd = __builtin_amdgcn_readlane(rec.second_dist, j);
            if (bi < 0 || bd > maxDist) continue;  // no candidate among the features free on entry, or none near enough: none now
            if (taken.test(bi)) {
                if (si < 0 || sd > maxDist) continue;  // the only candidate is taken, or nothing but the best was near enough on entry
                if (!taken.test(si)) {
                    bi = si; bd = sd;
                } else {
                    nResearched++;
                    const amos_best2 r = wave_research(a, fv, load_loop_query(a, lq, base + j), taken, lane);
                    if (r.best_idx < 0) continue;
                    bi = r.best_idx; bd = r.best_dist;
                }
                if (bd > maxDist) continue;  // :498 (a researched best; the recorded second has passed the test above)
            }
            nMatches++;
            if (lane == j) acc = bi;
            if (lane == 0) atomicOr(&taken.w[bi >> 5], 1u << (bi & 31));  // one LDS instruction, nothing returned
            __syncthreads();  // the bit is visible to every lane before the next point reads the bitmap
        }
        if (acc >= 0) loopMatch[acc] = i;  // a feature is accepted at most once by the call (outside the loop: a store there is waited for at every barrier)
    }
    const unsigned long long notFinite = __ballot(bad != 0);
    if (lane == 0) {
        amos_loop_points_stats s;
        s.n_candidates = nCandidates; s.n_in_view = nInView; s.n_matches = nMatches; s.n_researched = nResearched;
        s.n_total = nOccupied + nMatches; s.accepted = s.n_total >= lq.q.min_total ? 1 : 0;
        s.status = notFinite ? 1 : 0; s.skipped = 0;
        a.stats[k] = s;
    }
}

}  // namespace amos

using namespace amos;

// a query's own fields; hostScw: the record's Scw is the one the search reads
static bool loop_query_ok(const char *name, const amos_loop_points_query &q, bool hostScw, int k)
{
    if ((q.enabled != 0 && q.enabled != 1) || (q.found_from_match != 0 && q.found_from_match != 1)) {
        set_error("%s: query %d: enabled or found_from_match is neither 0 nor 1", name, k);
        return false;
    }
    if (q.max_dist < 0 || q.max_dist > 255) { set_error("%s: query %d: max_dist outside 0 .. 255", name, k); return false; }
    if (!(std::isfinite(q.th) && q.th > 0.f)) { set_error("%s: query %d: th is not finite or <= 0", name, k); return false; }
    if (!(std::isfinite(q.fx) && std::isfinite(q.fy) && std::isfinite(q.cx) && std::isfinite(q.cy))) {
        set_error("%s: query %d: the intrinsics are not finite", name, k);
        return false;
    }
    if (!hostScw) return true;
    bool ok = true;
    for (int i = 0; i < 16; i++) ok = ok && std::isfinite(q.Scw[i]);
    if (ok) {
        loop::Unscaled cw;
        loop::unscale(q.Scw, cw);
        ok = std::isfinite(cw.scw) && cw.scw > 0.f;
    }
    if (!ok) set_error("%s: query %d: Scw is not finite or its first row has norm 0", name, k);
    return ok;
}

extern "C" {

int amos_match_loop_points_batch_device(amos_match *m, const amos_loop_points_search *s)
{
    static const char *name = "amos_match_loop_points_batch_device";
    if (!m || !s || !s->d_kps || !s->d_desc || !s->d_counts || !s->d_cell_start || !s->d_items || !s->scale_factors || !s->d_points || !s->point_first ||
        !s->point_count || !s->queries || !s->d_matched || !s->d_loop_match || !s->d_stats || s->n_queries < 1 || s->n_frames < 1 || s->n_points < 0 ||
        s->capacity < 1 || s->capacity > 65536 || s->n_levels < 1 || s->n_levels > AMOS_MAX_LEVELS || !(s->max_x > s->min_x) || !(s->max_y > s->min_y)) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    int maxPoints = 0;
    size_t total = 0;
    bool fromMatch = false;
    std::vector<LoopQuery> queries((size_t)s->n_queries);
    for (int k = 0; k < s->n_queries; k++) {
        const amos_loop_points_query &q = s->queries[k];
        if (q.frame < 0 || q.frame >= s->n_frames) { set_error("%s: the frame of query %d lies outside n_frames", name, k); return AMOS_ERR_INVALID; }
        if (s->point_first[k] < 0 || s->point_count[k] < 0 || s->point_count[k] > s->n_points - s->point_first[k]) {
            set_error("%s: the point range of query %d lies outside n_points", name, k);
            return AMOS_ERR_INVALID;
        }
        if (!loop_query_ok(name, q, s->d_opt == nullptr, k)) return AMOS_ERR_INVALID;
        if (q.found_from_match && !s->d_point_of_feature2) { set_error("%s: query %d: found_from_match without d_point_of_feature2", name, k); return AMOS_ERR_INVALID; }
        fromMatch = fromMatch || (q.enabled && q.found_from_match);
        queries[k] = LoopQuery{q, s->point_first[k], s->point_count[k], (int)total};
        maxPoints = std::max(maxPoints, s->point_count[k]);
        total += (size_t)s->point_count[k];
        if (total > (size_t)INT_MAX) { set_error("%s: more than 2^31 - 1 points over all queries", name); return AMOS_ERR_INVALID; }
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    // the call's scratch: the query records, then per (query, point) the projection, the prepass record and the found byte
    const size_t oProj = align64(sizeof(LoopQuery) * queries.size()), oBest2 = oProj + align64(sizeof(LoopPoint) * total),
                 oFound = oBest2 + align64(sizeof(amos_best2) * total), bytes = oFound + align64(total);
    int rc = grow(&m->dLocal, &m->capLocal, bytes);
    if (rc != AMOS_OK) return rc;
    rc = upload_frames(m, queries.data(), sizeof(LoopQuery) * queries.size());
    if (rc != AMOS_OK) return rc;
    LoopArgs a;
    a.kps = s->d_kps; a.desc = s->d_desc; a.counts = s->d_counts; a.cellStart = s->d_cell_start; a.items = s->d_items; a.uRight = nullptr;
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.scale[l] = l < s->n_levels ? s->scale_factors[l] : 0.f;
    a.minX = s->min_x; a.maxX = s->max_x; a.minY = s->min_y; a.maxY = s->max_y;
    a.wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(s->max_x - s->min_x);  // Frame.cc:302-303
    a.hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(s->max_y - s->min_y);
    a.capacity = s->capacity; a.nLevels = s->n_levels;
    a.points = s->d_points; a.queries = (const LoopQuery *)m->dLocal; a.opt = s->d_opt; a.matched = s->d_matched; a.found = s->d_found;
    a.pointOfFeature2 = s->d_point_of_feature2; a.loopMatch = s->d_loop_match; a.stats = s->d_stats;
    a.proj = (LoopPoint *)(m->dLocal + oProj); a.best2 = (amos_best2 *)(m->dLocal + oBest2);
    a.foundMatch = fromMatch && total > 0 ? m->dLocal + oFound : nullptr;
    if (maxPoints > 0) {
        if (a.foundMatch) {
            AMOS_HIP_CHECK(hipMemsetAsync(a.foundMatch, 0, total, m->stream));
            hipLaunchKernelGGL(k_loop_found, dim3((s->capacity + 255) / 256, s->n_queries), dim3(256), 0, m->stream, a);
        }
        hipLaunchKernelGGL(k_loop_project, dim3((maxPoints + 255) / 256, s->n_queries), dim3(256), 0, m->stream, a);
        hipLaunchKernelGGL(k_loop_window_best2, window_grid(maxPoints, s->n_queries), dim3(256), 0, m->stream, a);
    }
    hipLaunchKernelGGL(k_loop_accept, dim3(s->n_queries), dim3(64), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_loop_points(amos_match *m, const amos_frame_view *kf, const amos_map_point *points, int n_points, const amos_loop_points_query *query,
                           const int32_t *matched, const uint8_t *found, const int32_t *point_of_feature2, int n2, const float *scale_factors,
                           int n_levels, int32_t *loop_match, amos_loop_points_stats *stats)
{
    static const char *name = "amos_match_loop_points";
    if (!m || !kf || !query || !scale_factors || !stats || n_points < 0 || (n_points > 0 && !points) || n2 < 0 || n2 > 65536 || (n2 > 0 && !point_of_feature2) ||
        kf->n < 0 || kf->n > 65536 || (kf->n > 0 && (!kf->keys_un || !kf->descriptors || !loop_match)) || n_levels < 1 || n_levels > AMOS_MAX_LEVELS ||
        !(kf->max_x > kf->min_x) || !(kf->max_y > kf->min_y) || query->frame != 0) {
        set_error("%s: invalid argument (a NULL pointer, a count or n_levels out of range, empty image bounds, or a frame other than 0)", name);
        return AMOS_ERR_INVALID;
    }
    if (!loop_query_ok(name, *query, true, 0)) return AMOS_ERR_INVALID;
    if (query->found_from_match && !point_of_feature2) { set_error("%s: found_from_match without point_of_feature2", name); return AMOS_ERR_INVALID; }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const int n = kf->n;
    const size_t cap = (size_t)std::max(std::max(n, n2), 1), np1 = (size_t)std::max(n_points, 1);
    // the download: loop_match [cap], the stats; then the grid
    const size_t oStats = align64(4 * cap), oEnd = oStats + align64(sizeof(amos_loop_points_stats)), oItems = oEnd + align64(4 * (kGridCells + 1)),
                 oAll = oItems + align64(4 * cap);
    int rc = stage_begin(m, cap * (sizeof(amos_keypoint) + 32 + 4 + 4 + 4) + np1 * (sizeof(amos_map_point) + 1) + 64 * 10 + oEnd);
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, oAll);
    if (rc != AMOS_OK) return rc;
    const float wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(kf->max_x - kf->min_x);
    const float hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(kf->max_y - kf->min_y);
    const size_t hKps = stage_take(m, cap * sizeof(amos_keypoint)), hDesc = stage_take(m, cap * 32), hCell = stage_take(m, cap * 4),
                 hRow = stage_take(m, cap * 4), hMap = stage_take(m, cap * 4), hCount = stage_take(m, 4);
    std::memset(m->hStage + hKps, 0, cap * sizeof(amos_keypoint));
    std::memset(m->hStage + hDesc, 0, cap * 32);
    int32_t *cell = (int32_t *)(m->hStage + hCell), *row = (int32_t *)(m->hStage + hRow), *map = (int32_t *)(m->hStage + hMap);
    std::fill(cell, cell + cap, -1);
    std::fill(row, row + cap, -1);
    std::fill(map, map + cap, -1);
    *(int32_t *)(m->hStage + hCount) = n;
    if (n) {
        std::memcpy(m->hStage + hKps, kf->keys_un, sizeof(amos_keypoint) * (size_t)n);
        std::memcpy(m->hStage + hDesc, kf->descriptors, 32 * (size_t)n);
        for (int i = 0; i < n; i++) cell[i] = pos_in_grid(kf->keys_un[i].x, kf->keys_un[i].y, kf->min_x, kf->min_y, wInv, hInv);
        if (matched) std::memcpy(row, matched, 4 * (size_t)n);
    }
    if (n2) std::memcpy(map, point_of_feature2, 4 * (size_t)n2);
    const std::vector<uint8_t> zeros(sizeof(amos_map_point), 0);
    const int32_t first = 0, count = n_points;
    uint8_t *out = (uint8_t *)m->dOut;
    amos_loop_points_search s;
    s.d_kps = (const amos_keypoint *)(m->dArena + hKps); s.d_desc = m->dArena + hDesc; s.d_counts = (const int32_t *)(m->dArena + hCount);
    s.d_cell_start = (int32_t *)(out + oEnd); s.d_items = (int32_t *)(out + oItems);
    s.scale_factors = scale_factors;
    s.d_points = stage_input<amos_map_point>(m, n_points ? (const void *)points : zeros.data(), sizeof(amos_map_point) * np1);
    s.point_first = &first; s.point_count = &count; s.queries = query; s.d_opt = nullptr;
    s.d_matched = (const int32_t *)(m->dArena + hRow);
    s.d_found = found && n_points ? stage_input<uint8_t>(m, found, (size_t)n_points) : nullptr;
    s.d_point_of_feature2 = (const int32_t *)(m->dArena + hMap);
    s.d_loop_match = (int32_t *)out; s.d_stats = (amos_loop_points_stats *)(out + oStats);
    s.n_frames = 1; s.n_queries = 1; s.n_points = n_points; s.capacity = (int32_t)cap; s.n_levels = n_levels;
    s.min_x = kf->min_x; s.max_x = kf->max_x; s.min_y = kf->min_y; s.max_y = kf->max_y;
    if ((rc = stage_flush(m)) != AMOS_OK ||
        (rc = amos_frame_grid_build_batch_device(m, (const int32_t *)(m->dArena + hCell), s.d_counts, 1, (int)cap, (int32_t *)(out + oEnd),
                                                 (int32_t *)(out + oItems))) != AMOS_OK ||
        (rc = amos_match_loop_points_batch_device(m, &s)) != AMOS_OK) return rc;
    const uint8_t *h = m->hStage + stage_take(m, oEnd);
    AMOS_HIP_CHECK(hipMemcpyAsync((void *)h, out, oEnd, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    std::memcpy(stats, h + oStats, sizeof(amos_loop_points_stats));
    if (!stats->skipped && n) std::memcpy(loop_match, h, 4 * (size_t)n);
    return AMOS_OK;
}

}  // extern "C"
