// amos_fuse.hip -- ORBmatcher::Fuse for a batch of (keyframe, point range, camera) PAIRS of resident keyframes: the pre-filter of
// ORBmatcher.cc:1042-1083 (projection, KeyFrame::IsInImage, distance invariance, the 60-degree test, MapPoint::PredictScale) and the search
// of :1085-1148 (KeyFrame::GetFeaturesInArea, the level gate, the chi-square gate, the nearest descriptor), in the local form
// Fuse(pKF, vpMapPoints, th) and in the loop-closing form Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1179-1312).
//
// ONE launch on the matcher's stream: k_fuse, eight lanes per (pair, point).  The search of a point reads only the keyframe's features, so
// there is no greedy stage and nothing a second launch would have to wait for: the eight lanes of a group each compute their point's
// projection (the same values in all eight: a few dozen operations against a window's descriptor loads) and walk every eighth grid column
// of its window; the group's first lane writes the record.  The arithmetic is defined in include/amos_frontend.h, "fuse search".
#include "amos_common.h"
#include "amos_projection_search.h"

#include "../../include/amos_host_types.h"  // amos_window_query, amos_frame_view

#include <vector>

namespace amos {

static_assert(sizeof(amos_fuse_camera) == 84, "amos_fuse_camera is 84 bytes (include/amos_frontend.h)");
static_assert(sizeof(amos_window_query) == 52, "amos_window_query is 52 bytes");
static_assert(sizeof(amos_fuse_stats) == 8, "amos_fuse_stats is 8 bytes");

struct FusePair {
    amos_fuse_camera cam;
    int frame, first, count, outOff;
};

struct FuseArgs : ProjArgs {
    float invSigma2[AMOS_MAX_LEVELS];
    const amos_map_point *points;
    const FusePair *pairs;
    const uint8_t *skip;
    amos_window_query *query;
    uint8_t *inView;
    int *bestIdx, *bestDist;
    amos_fuse_stats *stats;  // zeroed in front of the launch
    int chi2, maxDist;
};

// ---- grid = (ceil(max points of a pair * 8 / 256), pairs), block = 256.  No lane leaves before the group shuffles.
__global__ __launch_bounds__(256) void k_fuse(const FuseArgs a)
{
    const FusePair &pr = a.pairs[blockIdx.y];
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i = t / kWindowLanes, sub = t % kWindowLanes;
    const bool valid = i < pr.count;
    const amos_fuse_camera &c = pr.cam;
    const int f = pr.frame;
    const size_t o = (size_t)pr.outOff + (valid ? i : 0);
    WindowQuery q;
    q.u = q.v = q.ur = q.r = 0.f;
    q.lo = q.hi = 0;
    int level = 0;
    bool inView = false;
    const amos_map_point *mp = nullptr;
    if (valid) {
        mp = a.points + pr.first + i;
        const bool skipped = (mp->flags & AMOS_MAP_POINT_SKIP) || (a.skip && a.skip[o]);
        if (!skipped) {
            KeyframeProjection pj;
            if (keyframe_prefilter(a, c.Rcw, c.tcw, c.Ow, c.fx, c.fy, c.cx, c.cy, *mp, pj) == 0) {
                level = pj.level;
                q.u = pj.u; q.v = pj.v;
                q.ur = a.chi2 ? __fsub_rn(pj.u, __fmul_rn(c.mbf, pj.invz)) : 0.f;
                q.lo = level - 1; q.hi = level;
                q.r = __fmul_rn(c.th, a.scale[level]);
                q.d = load_desc_words(mp->desc);
                inView = true;
            }
        }
    }
    const bool active = inView && min(a.counts[f], a.capacity) > 0;
    FrameView fv = frame_view(a, f);
    const float *right = fv.tr;
    fv.tr = nullptr;  // the right-coordinate gate of window_candidate belongs to the frame searches; u_right is read by the chi-square test
    // the chi-square gate of :1106-1131 in float32, unfused, the product compared as a double; the level gate comes first, so the table is
    // read inside its range
    unsigned best, second;
    lanes_window_keys(a, fv, q, active, sub, kInitDist, [&](int idx) {
        if (!a.chi2) return true;
        const amos_keypoint k = fv.tk[idx];
        if (k.octave < q.lo || k.octave > q.hi || (unsigned)k.octave >= (unsigned)a.nLevels) return false;
        const float ex = __fsub_rn(q.u, k.x), ey = __fsub_rn(q.v, k.y);
        const float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
        const float kr = right ? right[idx] : -1.0f;
        if (kr >= 0) {
            const float er = __fsub_rn(q.ur, kr);
            return !((double)__fmul_rn(__fadd_rn(e2, __fmul_rn(er, er)), a.invSigma2[k.octave]) > 7.8);
        }
        return !((double)__fmul_rn(e2, a.invSigma2[k.octave]) > 5.99);
    }, best, second);
    const bool lead = valid && sub == 0;
    int bestIdx = -1, bestDist = kInitDist;
    if (best != 0xffffffffu) {
        bestDist = (int)(best >> 16);
        if (bestDist <= a.maxDist) bestIdx = fv.it[best & 0xffffu];
    }
    if (lead) {
        amos_window_query w;
        w.u = q.u; w.v = q.v; w.ur = q.ur;
        w.level = level; w.src = i;
        copy_desc(w.desc, mp->desc);
        a.query[o] = w;
        a.inView[o] = inView ? 1 : 0;
        a.bestIdx[o] = bestIdx;
        a.bestDist[o] = bestDist;
    }
    // per pair: the points in view and the accepted ones, counted per wave
    const unsigned long long seen = __ballot(lead && inView), got = __ballot(lead && bestIdx >= 0);
    if ((threadIdx.x & 63) == 0) {
        if (seen) atomicAdd(&a.stats[blockIdx.y].n_in_view, __popcll(seen));
        if (got) atomicAdd(&a.stats[blockIdx.y].n_accepted, __popcll(got));
    }
}

}  // namespace amos

using namespace amos;

extern "C" {

int amos_match_fuse_batch_device(amos_match *m, const amos_fuse_search *s)
{
    static const char *name = "amos_match_fuse_batch_device";
    if (!m || !s || !s->d_kps || !s->d_desc || !s->d_counts || !s->d_cell_start || !s->d_items || !s->d_points || !s->pair_frame || !s->point_first ||
        !s->point_count || !s->out_off || !s->cameras || !s->scale_factors || !s->d_query || !s->d_in_view || !s->d_best_idx || !s->d_best_dist ||
        !s->d_stats || s->n_frames < 1 || s->n_pairs < 1 || s->n_points < 0 || s->capacity < 1 || s->capacity > 65536 || s->n_levels < 1 ||
        s->n_levels > AMOS_MAX_LEVELS || !(s->max_x > s->min_x) || !(s->max_y > s->min_y) ||
        (s->mode != AMOS_FUSE_LOCAL && s->mode != AMOS_FUSE_SIM3) || (s->mode == AMOS_FUSE_LOCAL && !s->inv_level_sigma2)) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    int maxPoints = 0;
    for (int p = 0; p < s->n_pairs; p++) {
        if (s->pair_frame[p] < 0 || s->pair_frame[p] >= s->n_frames) { set_error("%s: pair_frame[%d] outside n_frames", name, p); return AMOS_ERR_INVALID; }
        if (s->point_first[p] < 0 || s->point_count[p] < 0 || s->point_count[p] > s->n_points - s->point_first[p]) {
            set_error("%s: the point range of pair %d lies outside n_points", name, p);
            return AMOS_ERR_INVALID;
        }
        if (s->out_off[p] < 0 || (p > 0 && s->out_off[p] - s->out_off[p - 1] < s->point_count[p - 1])) {
            set_error("%s: out_off out of order at %d", name, p);
            return AMOS_ERR_INVALID;
        }
        maxPoints = std::max(maxPoints, s->point_count[p]);
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t bytesPairs = sizeof(FusePair) * (size_t)s->n_pairs;
    int rc = grow(&m->dLocal, &m->capLocal, align64(bytesPairs));
    if (rc != AMOS_OK) return rc;
    std::vector<FusePair> pairs((size_t)s->n_pairs);
    for (int p = 0; p < s->n_pairs; p++) pairs[p] = FusePair{s->cameras[p], s->pair_frame[p], s->point_first[p], s->point_count[p], s->out_off[p]};
    rc = upload_frames(m, pairs.data(), bytesPairs);
    if (rc != AMOS_OK) return rc;
    FuseArgs a;
    fill_proj_args(a, *s);
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.invSigma2[l] = s->mode == AMOS_FUSE_LOCAL && l < s->n_levels ? s->inv_level_sigma2[l] : 0.f;
    a.points = s->d_points; a.pairs = (const FusePair *)m->dLocal; a.skip = s->d_skip;
    a.query = s->d_query; a.inView = s->d_in_view; a.bestIdx = s->d_best_idx; a.bestDist = s->d_best_dist; a.stats = s->d_stats;
    a.chi2 = s->mode == AMOS_FUSE_LOCAL ? 1 : 0; a.maxDist = s->max_dist;
    AMOS_HIP_CHECK(hipMemsetAsync(s->d_stats, 0, sizeof(amos_fuse_stats) * (size_t)s->n_pairs, m->stream));
    if (maxPoints > 0) {
        hipLaunchKernelGGL(k_fuse, window_grid(maxPoints, s->n_pairs), dim3(256), 0, m->stream, a);
        AMOS_HIP_CHECK(hipGetLastError());
    }
    return AMOS_OK;
}

int amos_match_fuse(amos_match *m, const amos_frame_view *kfs, int n_kfs, const amos_map_point *points, int n_points, int n_pairs,
                    const int32_t *pair_frame, const int32_t *point_first, const int32_t *point_count, const int32_t *out_off,
                    const amos_fuse_camera *cameras, const uint8_t *skip, int n_out, const float *scale_factors, const float *inv_level_sigma2,
                    int n_levels, int mode, int max_dist, struct amos_window_query *query, uint8_t *in_view, int32_t *best_idx, int32_t *best_dist,
                    amos_fuse_stats *stats)
{
    static const char *name = "amos_match_fuse";
    bool ok = m && n_kfs >= 0 && n_pairs >= 0 && n_points >= 0 && n_out >= 0 && (n_kfs == 0 || kfs) && (n_points == 0 || points) && scale_factors &&
              n_levels >= 1 && n_levels <= AMOS_MAX_LEVELS && (n_pairs == 0 || (n_kfs > 0 && pair_frame && point_first && point_count && out_off && cameras && stats)) &&
              (n_out == 0 || (query && in_view && best_idx && best_dist));
    int maxN = 0;
    bool anyRight = false;
    for (int k = 0; ok && k < n_kfs; k++) {
        const amos_frame_view &v = kfs[k];
        ok = v.n >= 0 && v.n <= 65536 && (v.n == 0 || (v.keys_un && v.descriptors)) && v.min_x == kfs[0].min_x && v.max_x == kfs[0].max_x &&
             v.min_y == kfs[0].min_y && v.max_y == kfs[0].max_y;
        maxN = std::max(maxN, v.n);
        anyRight |= v.n > 0 && v.u_right != nullptr;
    }
    for (int p = 0; ok && p < n_pairs; p++) ok = point_count[p] >= 0 && out_off[p] >= 0 && point_count[p] <= n_out - out_off[p];
    if (!ok) {
        set_error("%s: invalid argument (a NULL pointer, a count or n_levels out of range, keyframes with different image bounds, or outputs past n_out)", name);
        return AMOS_ERR_INVALID;
    }
    if (n_pairs == 0) return AMOS_OK;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t cap = (size_t)std::max(maxN, 1), nk = (size_t)n_kfs, np1 = (size_t)std::max(n_points, 1), no1 = (size_t)std::max(n_out, 1);
    const size_t oInView = align64(sizeof(amos_window_query) * no1), oIdx = oInView + align64(no1), oDist = oIdx + align64(4 * no1),
                 oStats = oDist + align64(4 * no1), oEnd = oStats + align64(sizeof(amos_fuse_stats) * (size_t)n_pairs),
                 oItems = oEnd + align64(4 * nk * (kGridCells + 1)), oAll = oItems + align64(4 * nk * cap);
    int rc = stage_begin(m, nk * cap * (sizeof(amos_keypoint) + 32 + 4 + 4) + 4 * nk + np1 * sizeof(amos_map_point) + no1 + 64 * 8 + oEnd);
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, oAll);
    if (rc != AMOS_OK) return rc;
    // every keyframe at the front of its slot of `cap` features, zeros behind; pos_in_grid on the way
    const float wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(kfs[0].max_x - kfs[0].min_x);
    const float hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(kfs[0].max_y - kfs[0].min_y);
    const size_t hKps = stage_take(m, nk * cap * sizeof(amos_keypoint)), hDesc = stage_take(m, nk * cap * 32), hCell = stage_take(m, nk * cap * 4);
    const size_t hRight = anyRight ? stage_take(m, nk * cap * 4) : 0, hCounts = stage_take(m, nk * 4);
    std::memset(m->hStage + hKps, 0, nk * cap * sizeof(amos_keypoint));
    std::memset(m->hStage + hDesc, 0, nk * cap * 32);
    int32_t *cell = (int32_t *)(m->hStage + hCell), *counts = (int32_t *)(m->hStage + hCounts);
    float *right = anyRight ? (float *)(m->hStage + hRight) : nullptr;
    std::fill(cell, cell + nk * cap, -1);
    if (right) std::fill(right, right + nk * cap, -1.0f);
    for (size_t k = 0; k < nk; k++) {
        const amos_frame_view &v = kfs[k];
        counts[k] = v.n;
        if (!v.n) continue;
        std::memcpy(m->hStage + hKps + k * cap * sizeof(amos_keypoint), v.keys_un, sizeof(amos_keypoint) * (size_t)v.n);
        std::memcpy(m->hStage + hDesc + k * cap * 32, v.descriptors, 32 * (size_t)v.n);
        if (right && v.u_right) std::memcpy(right + k * cap, v.u_right, 4 * (size_t)v.n);
        for (int i = 0; i < v.n; i++) cell[k * cap + i] = pos_in_grid(v.keys_un[i].x, v.keys_un[i].y, v.min_x, v.min_y, wInv, hInv);
    }
    const std::vector<uint8_t> zeros(sizeof(amos_map_point), 0);
    uint8_t *out = (uint8_t *)m->dOut;
    amos_fuse_search s;
    s.d_kps = (const amos_keypoint *)(m->dArena + hKps); s.d_desc = m->dArena + hDesc; s.d_counts = (const int32_t *)(m->dArena + hCounts);
    s.d_cell_start = (int32_t *)(out + oEnd); s.d_items = (int32_t *)(out + oItems);
    s.d_u_right = anyRight ? (const float *)(m->dArena + hRight) : nullptr;
    s.d_points = stage_input<amos_map_point>(m, n_points ? (const void *)points : zeros.data(), sizeof(amos_map_point) * np1);
    s.d_skip = skip && n_out ? stage_input<uint8_t>(m, skip, (size_t)n_out) : nullptr;
    s.pair_frame = pair_frame; s.point_first = point_first; s.point_count = point_count; s.out_off = out_off; s.cameras = cameras;
    s.scale_factors = scale_factors; s.inv_level_sigma2 = inv_level_sigma2;
    s.d_query = (amos_window_query *)out; s.d_in_view = out + oInView; s.d_best_idx = (int32_t *)(out + oIdx); s.d_best_dist = (int32_t *)(out + oDist);
    s.d_stats = (amos_fuse_stats *)(out + oStats);
    s.n_frames = n_kfs; s.n_pairs = n_pairs; s.n_points = n_points; s.capacity = (int32_t)cap; s.n_levels = n_levels; s.mode = mode; s.max_dist = max_dist;
    s.min_x = kfs[0].min_x; s.max_x = kfs[0].max_x; s.min_y = kfs[0].min_y; s.max_y = kfs[0].max_y;
    if ((rc = stage_flush(m)) != AMOS_OK ||
        (rc = amos_frame_grid_build_batch_device(m, (const int32_t *)(m->dArena + hCell), s.d_counts, n_kfs, (int)cap, (int32_t *)(out + oEnd),
                                                 (int32_t *)(out + oItems))) != AMOS_OK ||
        (rc = amos_match_fuse_batch_device(m, &s)) != AMOS_OK) return rc;
    const uint8_t *h = m->hStage + stage_take(m, oEnd);
    AMOS_HIP_CHECK(hipMemcpyAsync((void *)h, out, oEnd, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    for (int p = 0; p < n_pairs; p++) {
        const size_t o = (size_t)out_off[p], c = (size_t)point_count[p];
        if (!c) continue;
        std::memcpy(query + o, h + sizeof(amos_window_query) * o, sizeof(amos_window_query) * c);
        std::memcpy(in_view + o, h + oInView + o, c);
        std::memcpy(best_idx + o, h + oIdx + 4 * o, 4 * c);
        std::memcpy(best_dist + o, h + oDist + 4 * o, 4 * c);
    }
    std::memcpy(stats, h + oStats, sizeof(amos_fuse_stats) * (size_t)n_pairs);
    return AMOS_OK;
}

}  // extern "C"
