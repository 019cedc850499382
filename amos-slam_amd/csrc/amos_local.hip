// amos_local.hip -- step 2 of Tracking::SearchLocalPoints (Tracking.cc:2352-2389) for a batch of resident frames: Frame::isInFrustum
// (Frame.cc:761-891) with MapPoint::PredictScale (MapPoint.cc:571-586) on every local map point, then
// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (ORBmatcher.cc:70-175) over the points in view.
//
// Three launches on the matcher's stream: k_local_frustum (one thread per point), k_local_window_best2 (eight lanes per point in view:
// the best two features of its window as the frame stands on entry) and k_local_accept (one wave per frame: the reference's sequential
// greedy loop over those records).  The arithmetic is defined in include/amos_frontend.h, "local map search".
#include "amos_common.h"
#include "amos_projection_search.h"

#include "../../include/amos_host_types.h"  // amos_map_query

#include <vector>

namespace amos {

static_assert(sizeof(amos_map_point) == 80, "amos_map_point is 80 bytes (include/amos_frontend.h)");
static_assert(sizeof(amos_local_camera) == 92, "amos_local_camera is 92 bytes");
static_assert(sizeof(amos_map_query) == 56, "amos_map_query is 56 bytes");

struct LocalFrame {
    amos_local_camera cam;
    int off0, off1;  // the frame's points
};

struct LocalArgs : ProjArgs {
    const amos_map_point *points;
    const LocalFrame *frames;
    const uint8_t *occupied;
    amos_map_query *query;
    uint8_t *inView;
    int *match;
    amos_local_stats *stats;
    amos_best2 *best2;  // scratch, one per point
    uint8_t *flags;     // scratch, one per point: bit 0 in view, bit 1 a projection that is not finite
};

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
    copy_desc(q.desc, mp.desc);
    int flags = 0;
    if (!(mp.flags & AMOS_MAP_POINT_SKIP)) {
        float PcX, PcY, PcZ;
        camera_point(c.Rcw, c.tcw, mp.pos, PcX, PcY, PcZ);
        if (!(PcZ < 0.0f)) {
            const float invz = __fdiv_rn(1.0f, PcZ);
            const float u = __fadd_rn(__fmul_rn(__fmul_rn(c.fx, PcX), invz), c.cx);
            const float v = __fadd_rn(__fmul_rn(__fmul_rn(c.fy, PcY), invz), c.cy);
            if (pixel_in_bounds(a, u, v, flags)) {
                float PO[3];
                const float dist = point_offset(mp.pos, c.Ow, PO);
                if (in_distance_band(dist, mp.min_distance, mp.max_distance)) {
                    const float viewCos = (float)__ddiv_rn(normal_dot(PO, mp.normal), (double)dist);
                    if (!(viewCos < c.view_cos_limit)) {
                        q.proj_x = u; q.proj_y = v;
                        q.proj_xr = __fsub_rn(u, __fmul_rn(c.mbf, invz));
                        q.view_cos = viewCos;
                        q.level = predict_scale_level(a, mp.max_distance, dist);
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
__device__ __forceinline__ WindowQuery load_local_query(const LocalArgs &a, const amos_local_camera &c, int p)
{
    const amos_map_query &q = a.query[p];
    WindowQuery o;
    o.u = q.proj_x; o.v = q.proj_y; o.ur = q.proj_xr;
    o.lo = q.level - 1; o.hi = q.level;  // bCheckLevels holds: maxLevel = level >= 0 (Frame.cc:945)
    float r = (double)q.view_cos > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos, ORBmatcher.cc:178-184: a comparison in double
    if (c.th != 1.0f) r = __fmul_rn(r, c.th);
    o.r = __fmul_rn(r, a.scale[q.level]);
    o.d = load_desc_words(q.desc);
    return o;
}

// ---- the window search of ORBmatcher.cc:93-160 against the frame as it stands on entry (d_occupied).
// grid = (ceil(max points * 8 / 256), frames), block = 256.
__global__ __launch_bounds__(256) void k_local_window_best2(const LocalArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    const LocalFrame &fr = a.frames[f];
    const int p = fr.off0 + t / kWindowLanes;
    const bool active = p < fr.off1 && a.inView[p] != 0 && min(a.counts[f], a.capacity) > 0;
    WindowQuery q;
    if (active) q = load_local_query(a, fr.cam, p);
    const uint8_t *occ = a.occupied + (size_t)f * a.capacity;
    lanes_window_best2(a, frame_view(a, f), q, active, t % kWindowLanes, kInitDist, [&](int idx) { return occ[idx] == 0; },
                       p < fr.off1 ? a.best2 + p : nullptr);
}

// ---- the greedy loop of ORBmatcher.cc:77-172.  One wave per frame walks the points in list order with a bitmap of the taken features
// in LDS (on entry: d_occupied).  A point whose two best features are both still free keeps its record: removing OTHER candidates
// cannot change the top two.  Otherwise the whole wave searches the point's window again against the bitmap.
// Everything the branches read is wave-uniform (read from one lane), so the barriers are reached by all lanes.
__global__ __launch_bounds__(64) void k_local_accept(const LocalArgs a)
{
    __shared__ TakenBitmap taken;
    const int f = blockIdx.x, lane = threadIdx.x;
    const LocalFrame &fr = a.frames[f];
    const int cap = a.capacity;
    const int off0 = fr.off0, off1 = fr.off1;
    const float nnRatio = fr.cam.nn_ratio;
    const FrameView fv = frame_view(a, f);
    const uint8_t *occ = a.occupied + (size_t)f * cap;
    int *match = a.match + (size_t)f * cap;
    for (int base = 0; base < cap; base += 64) {  // base / 32 + 1 < kTakenWords: cap <= 65536
        const int i = base + lane;
        const unsigned long long m = __ballot(i < cap && occ[i] != 0);
        if (lane == 0) {
            taken.w[base >> 5] = (uint32_t)m;
            taken.w[(base >> 5) + 1] = (uint32_t)(m >> 32);
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
        amos_best2 rec = best2_from_keys(0xffffffffu, 0xffffffffu, nullptr, kInitDist);  // none
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
            amos_best2 r;
            r.best_idx = __builtin_amdgcn_readlane(rec.best_idx, k); r.best_dist = __builtin_amdgcn_readlane(rec.best_dist, k);
            r.second_idx = __builtin_amdgcn_readlane(rec.second_idx, k); r.second_dist = __builtin_amdgcn_readlane(rec.second_dist, k);
            const int ho = __builtin_amdgcn_readlane(hasObs, k);
            if (r.best_idx < 0) continue;  // no candidate on entry: none now
            if (taken.either(r.best_idx, r.second_idx)) {
                nResearched++;
                r = wave_research(a, fv, load_local_query(a, fr.cam, base + k), taken, lane);
            }
            if (r.best_idx < 0 || r.best_dist > AMOS_TH_HIGH) continue;
            const int bestLevel = fv.tk[r.best_idx].octave, bestLevel2 = r.second_idx >= 0 ? fv.tk[r.second_idx].octave : -1;
            if (bestLevel == bestLevel2 && (float)r.best_dist > __fmul_rn(nnRatio, (float)r.second_dist)) continue;
            nMatches++;
            if (lane == 0) {
                match[r.best_idx] = base + k - off0;
                if (ho) taken.set(r.best_idx);
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

extern "C" {

int amos_match_local_points_batch_device(amos_match *m, const amos_local_search *s)
{
    int maxPoints;
    size_t total;
    int rc = check_point_search("amos_match_local_points_batch_device", m, s, s && s->d_occupied && s->d_in_view, &maxPoints, &total);
    if (rc != AMOS_OK) return rc;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const PointScratch l = point_scratch(sizeof(LocalFrame) * (size_t)s->n_frames, total, false, 1);
    rc = grow(&m->dLocal, &m->capLocal, l.bytes);
    if (rc != AMOS_OK) return rc;
    std::vector<LocalFrame> frames((size_t)s->n_frames);
    for (int f = 0; f < s->n_frames; f++) frames[f] = LocalFrame{s->cameras[f], s->point_off[f], s->point_off[f + 1]};
    rc = upload_frames(m, frames.data(), sizeof(LocalFrame) * frames.size());
    if (rc != AMOS_OK) return rc;
    LocalArgs a;
    fill_proj_args(a, *s);
    a.points = s->d_points; a.frames = (const LocalFrame *)m->dLocal; a.occupied = s->d_occupied;
    a.query = s->d_query; a.inView = s->d_in_view; a.match = s->d_match; a.stats = s->d_stats;
    a.best2 = (amos_best2 *)(m->dLocal + l.best2); a.flags = m->dLocal + l.flags;
    if (maxPoints > 0) {
        hipLaunchKernelGGL(k_local_frustum, dim3((maxPoints + 255) / 256, s->n_frames), dim3(256), 0, m->stream, a);
        hipLaunchKernelGGL(k_local_window_best2, window_grid(maxPoints, s->n_frames), dim3(256), 0, m->stream, a);
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
    const size_t cap = (size_t)std::max(n, 1), np1 = (size_t)std::max(n_points, 1);
    return one_frame_search<amos_local_search>(m, amos_match_local_points_batch_device, kps_un, desc, u_right, n, n_points, cap + 64 + np1 * sizeof(amos_map_point), scale_factors,
                                               n_levels, min_x, max_x, min_y, max_y, query, in_view, match, stats,
                                               [&](amos_local_search &s, uint8_t *d_flag, const uint8_t *zeros) {
        s.d_occupied = stage_input<uint8_t>(m, n ? occupied : zeros, cap);
        s.d_points = stage_input<amos_map_point>(m, n_points ? (const void *)points : zeros, sizeof(amos_map_point) * np1);
        s.cameras = camera;
        s.d_in_view = d_flag;
    });
}

}  // extern "C"
