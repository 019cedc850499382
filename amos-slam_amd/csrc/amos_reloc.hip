// amos_reloc.hip -- step 6 of Tracking::Relocalization's candidate loop (Tracking.cc:2732, :2756) for a batch of pairs (current frame,
// candidate keyframe) on resident frames: ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
// (ORBmatcher.cc:1731-1863).
//
// Launches on the matcher's stream: k_reloc_found (only when a pair has found_from_match: one thread per feature marks the point its
// entry match names), k_reloc_project (one thread per keyframe point), k_reloc_window_best2 (eight lanes per projected point: the best two
// features of its window among those free on entry) and k_reloc_accept (one wave per pair: the reference's sequential greedy loop over
// those records, then the rotation histogram's pruning).  The arithmetic is defined in include/amos_frontend.h, "relocalisation search".
#include "amos_common.h"
#include "amos_projection_search.h"

#include "../../include/amos_host_types.h"  // amos_kf_query

#include <vector>

namespace amos {

static_assert(sizeof(amos_reloc_point) == 64 && offsetof(amos_reloc_point, flags) == 24, "amos_reloc_point is 64 bytes, flags at 24 (include/amos_frontend.h)");
static_assert(sizeof(amos_reloc_camera) == 84, "amos_reloc_camera is 84 bytes");
static_assert(sizeof(amos_reloc_stats) == 32, "amos_reloc_stats is 32 bytes");
static_assert(sizeof(amos_kf_query) == 48, "amos_kf_query is 48 bytes");
static_assert(sizeof(amos_pose_result) == 272, "amos_pose_result is 272 bytes");
static_assert(AMOS_HISTO_LENGTH <= 64, "one lane per histogram bin");

struct RelocPair {
    amos_reloc_camera cam;
    float Ow[3];     // -Rcw^T tcw of the camera's pose (not read when the pose comes from d_pose)
    int frame;       // whose keypoints, descriptors and grid the pair searches
    int off0, off1;  // the pair's points
};

struct RelocArgs : ProjArgs {
    const amos_reloc_point *points;
    const RelocPair *pairs;
    const uint8_t *found;          // one per point, or null
    const amos_pose_result *pose;  // one per pair, or null: the cameras' poses
    amos_kf_query *query;
    uint8_t *projected;
    int *match;                    // [pairs][capacity]
    amos_reloc_stats *stats;
    amos_best2 *best2;    // scratch, one per point
    int *accepted;        // scratch, one per point: -1, or bin << 16 | feature of the point's accepted match
    uint8_t *flags;       // scratch, one per point: bit 0 projected, bit 1 a projection that is not finite, bit 2 candidate, bit 3 found
    uint8_t *foundMatch;  // scratch, one per point (zeroed by the entry): 1 where an entry match names the point; null: no pair asks
};
enum { kProjected = 1, kNotFinite = 2, kCandidate = 4, kFound = 8 };

// ---- the rebuild of sFound from the frame's matches (Tracking.cc:2752-2755).  grid = (ceil(capacity / 256), pairs), block = 256.
__global__ __launch_bounds__(256) void k_reloc_found(const RelocArgs a)
{
    const RelocPair &pr = a.pairs[blockIdx.y];
    if (!pr.cam.enabled || !pr.cam.found_from_match) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(a.counts[pr.frame], a.capacity)) return;
    const int j = a.match[(size_t)blockIdx.y * a.capacity + i];
    if (j >= 0 && j < pr.off1 - pr.off0) a.foundMatch[pr.off0 + j] = 1;  // several features of one point write the same value
}

// ---- the projection of ORBmatcher.cc:1750-1788.  grid = (ceil(max points of a pair / 256), pairs), block = 256.
__global__ __launch_bounds__(256) void k_reloc_project(const RelocArgs a)
{
    const RelocPair &pr = a.pairs[blockIdx.y];
    if (!pr.cam.enabled) return;
    const int p = pr.off0 + blockIdx.x * 256 + threadIdx.x;
    if (p >= pr.off1) return;
    const amos_reloc_camera &c = pr.cam;
    const amos_reloc_point &kp = a.points[p];
    amos_kf_query q;
    q.u = q.v = 0.f;
    q.level = 0;
    q.angle = kp.angle;
    copy_desc(q.desc, kp.desc);
    int flags = 0;
    if (!(kp.flags & AMOS_RELOC_POINT_SKIP)) {
        const bool found = (a.found && a.found[p] != 0) || (c.found_from_match && a.foundMatch[p] != 0);
        if (found) flags = kFound;
        else {
            flags = kCandidate;
            float R[9], t[3], Ow[3];
            if (a.pose) {
                const amos_pose_result &po = a.pose[blockIdx.y];
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    R[3 * r] = po.Tcw[4 * r]; R[3 * r + 1] = po.Tcw[4 * r + 1]; R[3 * r + 2] = po.Tcw[4 * r + 2];
                    t[r] = po.Tcw[4 * r + 3];
                    Ow[r] = po.Ow[r];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 9; k++) R[k] = c.Rcw[k];
#pragma unroll
                for (int r = 0; r < 3; r++) { t[r] = c.tcw[r]; Ow[r] = pr.Ow[r]; }
            }
            float xc, yc, zc;
            camera_point(R, t, kp.pos, xc, yc, zc);
            const float invzc = (float)__ddiv_rn(1.0, (double)zc);  // no sign test: :1762-1770
            const float u = __fadd_rn(__fmul_rn(__fmul_rn(c.fx, xc), invzc), c.cx);
            const float v = __fadd_rn(__fmul_rn(__fmul_rn(c.fy, yc), invzc), c.cy);
            if (pixel_in_bounds(a, u, v, flags)) {
                float PO[3];
                const float dist = point_offset(kp.pos, Ow, PO);
                if (in_distance_band(dist, kp.min_distance, kp.max_distance)) {
                    q.u = u; q.v = v;
                    q.level = predict_scale_level(a, kp.max_distance, dist);
                    flags |= kProjected;
                }
            }
        }
    }
    a.query[p] = q;
    a.projected[p] = (uint8_t)(flags & kProjected);
    a.flags[p] = (uint8_t)flags;
}

// what the search reads of one projected point
__device__ __forceinline__ WindowQuery load_reloc_query(const RelocArgs &a, const RelocPair &pr, int p)
{
    const amos_kf_query &q = a.query[p];
    WindowQuery o;
    o.u = q.u; o.v = q.v; o.ur = 0.f;  // no right gate: the frame view has no right coordinates
    o.r = __fmul_rn(pr.cam.th, a.scale[q.level]);
    level_window(o, q.level, false, false);
    o.d = load_desc_words(q.desc);
    return o;
}

// ---- the candidate loop of ORBmatcher.cc:1791-1816 against the frame as it stands on entry: the best two of the features that are free
// then.  grid = (ceil(max points * 8 / 256), pairs), block = 256.
__global__ __launch_bounds__(256) void k_reloc_window_best2(const RelocArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    const RelocPair &pr = a.pairs[k];
    if (!pr.cam.enabled) return;  // the whole work-group
    const int p = pr.off0 + t / kWindowLanes;
    const bool active = p < pr.off1 && a.projected[p] != 0 && min(a.counts[pr.frame], a.capacity) > 0;
    WindowQuery q;
    if (active) q = load_reloc_query(a, pr, p);
    const int *matchOnEntry = a.match + (size_t)k * a.capacity;  // k_reloc_accept, the only writer, runs behind this launch
    lanes_window_best2(a, frame_view(a, pr.frame), q, active, t % kWindowLanes, kInitDist, [&](int idx) { return matchOnEntry[idx] < 0; },
                       p < pr.off1 ? a.best2 + p : nullptr);
}

// ---- the sequential loop of ORBmatcher.cc:1748-1839 and the pruning of :1841-1860.  One wave per pair walks the points in list order
// with a bitmap of the set features in LDS (on entry: d_match >= 0).  Every accept sets its bit, so a feature is matched at most once by
// the call.  The prepass record decides each point: best free -> the best; best taken and second free -> the second (the minimum of
// everything but the best, and it is free); both taken -> the whole wave searches the window again against the bitmap.  Every accepted
// point is one histogram entry (its feature and bin are kept per point in a.accepted), so the pruning reaches this call's matches only;
// d_match itself is written behind the loop from those entries.
// Everything the branches read is wave-uniform (read from one lane, or from LDS behind a barrier), so the barriers are reached by all lanes.
__global__ __launch_bounds__(64) void k_reloc_accept(const RelocArgs a)
{
    __shared__ TakenBitmap taken;
    __shared__ int hist[AMOS_HISTO_LENGTH];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const RelocPair &pr = a.pairs[pair];
    if (!pr.cam.enabled) {  // the whole wave
        if (lane == 0) {
            amos_reloc_stats s = {};
            s.skipped = 1;
            a.stats[pair] = s;
        }
        return;
    }
    const int cap = a.capacity, count = min(a.counts[pr.frame], cap);
    const int off0 = pr.off0, off1 = pr.off1;
    const bool checkOri = pr.cam.check_orientation != 0;
    const int orbDist = pr.cam.orb_dist;
    const FrameView fv = frame_view(a, pr.frame);
    int *match = a.match + (size_t)pair * cap;
    int nOccupied = 0;
    for (int base = 0; base < cap; base += 64) {  // base / 32 + 1 < kTakenWords: cap <= 65536
        const int i = base + lane;
        const bool set = i < cap && match[i] >= 0;
        const unsigned long long m = __ballot(set);
        nOccupied += __popcll(__ballot(set && i < count));
        if (lane == 0) {
            taken.w[base >> 5] = (uint32_t)m;
            taken.w[(base >> 5) + 1] = (uint32_t)(m >> 32);
        }
    }
    __syncthreads();
    int myBin = 0;  // the histogram: lane b holds the entries of bin b
    int nCandidates = 0, nFound = 0, nProjected = 0, nMatches = 0, nResearched = 0, bad = 0;
    for (int base = off0; base < off1; base += 64) {
        const int p = base + lane;
        const bool valid = p < off1;
        const int fl = valid ? a.flags[p] : 0;
        bad |= fl & kNotFinite;
        nCandidates += __popcll(__ballot((fl & kCandidate) != 0));
        nFound += __popcll(__ballot((fl & kFound) != 0));
        amos_best2 rec = best2_from_keys(0xffffffffu, 0xffffffffu, nullptr, kInitDist);  // none
        float angle = 0.f, bestAngle = 0.f, secondAngle = 0.f;
        if (fl & kProjected) {
            rec = a.best2[p];
            angle = a.query[p].angle;
            if (checkOri) {  // the two features' angles travel with the record: no global load inside the sequential loop
                if (rec.best_idx >= 0) bestAngle = fv.tk[rec.best_idx].angle;
                if (rec.second_idx >= 0) secondAngle = fv.tk[rec.second_idx].angle;
            }
        }
        int acc = -1;  // this lane's point: bin << 16 | feature once it is accepted
        unsigned long long todo = __ballot((fl & kProjected) != 0);
        nProjected += __popcll(todo);
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1;
            int bi = __builtin_amdgcn_readlane(rec.best_idx, k), bd = __builtin_amdgcn_readlane(rec.best_dist, k);
            const int si = __builtin_amdgcn_readlane(rec.second_idx, k), sd = __builtin_amdgcn_readlane(rec.second_dist, k);
            float featAngle = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bestAngle), k));
            if (bi < 0) continue;  // no candidate among the features free on entry: none now
            if (taken.test(bi)) {
                if (si < 0) continue;  // the only candidate is taken
                if (!taken.test(si)) {
                    bi = si; bd = sd;
                    featAngle = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(secondAngle), k));
                } else {
                    nResearched++;
                    const amos_best2 r = wave_research(a, fv, load_reloc_query(a, pr, base + k), taken, lane);
                    if (r.best_idx < 0) continue;
                    bi = r.best_idx; bd = r.best_dist;
                    if (checkOri) featAngle = fv.tk[bi].angle;
                }
            }
            if (bd > orbDist) continue;  // :1818
            nMatches++;
            int bin = 0;
            if (checkOri) bin = rotation_bin(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(angle), k)), featAngle);  // :1824-1834
            if (lane == k) acc = (bin << 16) | bi;
            myBin += (checkOri && lane == bin) ? 1 : 0;  // lane b counts bin b (AMOS_HISTO_LENGTH <= 64): no LDS round trip
            if (lane == 0) atomicOr(&taken.w[bi >> 5], 1u << (bi & 31));  // one LDS instruction, nothing returned
            __syncthreads();  // the bit is visible to every lane before the next point reads the bitmap
        }
        if (valid) a.accepted[p] = acc;  // (read back below by the lane that writes it)
    }
    if (lane < AMOS_HISTO_LENGTH) hist[lane] = myBin;
    __syncthreads();
    // d_match is written here, not inside the loop (a store there is waited for at every barrier): a feature is accepted at most once by
    // the call, so the order of these stores does not matter; an entry of a losing bin leaves its feature at -1 (:1849-1858)
    int ind1 = -1, ind2 = -1, ind3 = -1;
    if (checkOri) three_maxima(hist, ind1, ind2, ind3);
    int pruned = 0;
    for (int base = off0; base < off1; base += 64) {
        const int p = base + lane;
        const int acc = p < off1 ? a.accepted[p] : -1;
        const int bin = acc >> 16;
        const bool lose = checkOri && acc >= 0 && bin != ind1 && bin != ind2 && bin != ind3;
        if (acc >= 0) match[acc & 0xffff] = lose ? -1 : p - off0;
        pruned += __popcll(__ballot(lose));
    }
    nMatches -= pruned;
    const unsigned long long notFinite = __ballot(bad != 0);
    if (lane == 0) {
        amos_reloc_stats s;
        s.n_candidates = nCandidates; s.n_projected = nProjected; s.n_matches = nMatches; s.n_researched = nResearched;
        s.n_found = nFound; s.n_occupied = nOccupied; s.status = notFinite ? 1 : 0; s.skipped = 0;
        a.stats[pair] = s;
    }
}

}  // namespace amos

using namespace amos;

extern "C" {

int amos_match_reloc_batch_device(amos_match *m, const amos_reloc_search *s)
{
    static const char *name = "amos_match_reloc_batch_device";
    int maxPoints;
    size_t total;
    int rc = check_point_search(name, m, s, s && s->frame_of_pair && s->d_projected && s->n_pairs >= 1, &maxPoints, &total, &amos_reloc_search::n_pairs,
                                &amos_reloc_search::frame_of_pair);
    if (rc != AMOS_OK) return rc;
    bool fromMatch = false;
    for (int k = 0; k < s->n_pairs; k++) {
        const amos_reloc_camera &c = s->cameras[k];
        if (c.orb_dist < 0 || c.orb_dist > 255) { set_error("%s: orb_dist of pair %d outside 0 .. 255", name, k); return AMOS_ERR_INVALID; }
        if (!std::isfinite(c.th) || !(c.th > 0.f)) { set_error("%s: th of pair %d is not finite and positive", name, k); return AMOS_ERR_INVALID; }
        fromMatch = fromMatch || (c.enabled && c.found_from_match);
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const PointScratch l = point_scratch(sizeof(RelocPair) * (size_t)s->n_pairs, total, true, 2);
    rc = grow(&m->dLocal, &m->capLocal, l.bytes);
    if (rc != AMOS_OK) return rc;
    std::vector<RelocPair> pairs((size_t)s->n_pairs);
    for (int k = 0; k < s->n_pairs; k++) {
        RelocPair &pr = pairs[k];
        pr.cam = s->cameras[k];
        pr.frame = s->frame_of_pair[k]; pr.off0 = s->point_off[k]; pr.off1 = s->point_off[k + 1];
        camera_centre(pr.cam.Rcw, pr.cam.tcw, pr.Ow);
    }
    rc = upload_frames(m, pairs.data(), sizeof(RelocPair) * pairs.size());
    if (rc != AMOS_OK) return rc;
    RelocArgs a;
    fill_proj_args(a, *s, nullptr);
    a.points = s->d_points; a.pairs = (const RelocPair *)m->dLocal; a.found = s->d_found; a.pose = s->d_pose;
    a.query = s->d_query; a.projected = s->d_projected; a.match = s->d_match; a.stats = s->d_stats;
    a.best2 = (amos_best2 *)(m->dLocal + l.best2); a.accepted = (int *)(m->dLocal + l.accepted); a.flags = m->dLocal + l.flags;
    a.foundMatch = fromMatch && total > 0 ? m->dLocal + l.flags2 : nullptr;
    if (maxPoints > 0) {
        if (a.foundMatch) {
            AMOS_HIP_CHECK(hipMemsetAsync(a.foundMatch, 0, total, m->stream));
            hipLaunchKernelGGL(k_reloc_found, dim3((s->capacity + 255) / 256, s->n_pairs), dim3(256), 0, m->stream, a);
        }
        hipLaunchKernelGGL(k_reloc_project, dim3((maxPoints + 255) / 256, s->n_pairs), dim3(256), 0, m->stream, a);
        hipLaunchKernelGGL(k_reloc_window_best2, window_grid(maxPoints, s->n_pairs), dim3(256), 0, m->stream, a);
    }
    hipLaunchKernelGGL(k_reloc_accept, dim3(s->n_pairs), dim3(64), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_reloc(amos_match *m, const amos_keypoint *kps_un, const uint8_t *desc, int n, const amos_reloc_point *points, int n_points,
                     const uint8_t *found, const amos_reloc_camera *camera, const float *scale_factors, int n_levels, float min_x,
                     float max_x, float min_y, float max_y, struct amos_kf_query *query, uint8_t *projected, int32_t *match,
                     amos_reloc_stats *stats)
{
    if (!m || !camera || !scale_factors || !stats || n < 0 || n > 65536 || n_points < 0 || (n > 0 && (!kps_un || !desc || !match)) ||
        (n_points > 0 && (!points || !query || !projected)) || n_levels < 1 || n_levels > AMOS_MAX_LEVELS || !(max_x > min_x) || !(max_y > min_y) ||
        camera->orb_dist < 0 || camera->orb_dist > 255 || !std::isfinite(camera->th) || !(camera->th > 0.f)) {
        set_error("amos_match_reloc: invalid argument");
        return AMOS_ERR_INVALID;
    }
    const size_t np1 = (size_t)std::max(n_points, 1);
    const int32_t frameOfPair = 0;
    return one_frame_search<amos_reloc_search>(m, amos_match_reloc_batch_device, kps_un, desc, nullptr, n, n_points,
                                              np1 * (sizeof(amos_reloc_point) + 1) + 128, scale_factors, n_levels, min_x, max_x, min_y, max_y,
                                              query, projected, match, stats, [&](amos_reloc_search &s, uint8_t *d_flag, const uint8_t *zeros) {
        s.d_points = stage_input<amos_reloc_point>(m, n_points ? (const void *)points : zeros, sizeof(amos_reloc_point) * np1);
        s.d_found = found && n_points ? stage_input<uint8_t>(m, found, np1) : nullptr;
        s.d_pose = nullptr;
        s.frame_of_pair = &frameOfPair;
        s.cameras = camera;
        s.d_projected = d_flag;
    }, true);
}

}  // extern "C"
