// amos_motion.hip -- Tracking::TrackWithMotionModel's search (Tracking.cc:1925-1945) for a batch of resident frames: the fill of
// mvpMapPoints, ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1569-1728) and the second search with the
// doubled radius when the first found fewer than 20 matches.
//
// Launches on the matcher's stream: k_motion_project (one thread per last-frame point), k_motion_window_best2 (eight lanes per projected
// point: the best two features of its window in the EMPTY frame) and k_motion_accept (one wave per frame: the reference's sequential
// greedy loop over those records, then the rotation histogram's pruning); the last two once more with th_retry, where every work-group
// of a frame whose first search found enough returns at once.  The arithmetic is defined in include/amos_frontend.h, "motion-model search".
#include "amos_common.h"
#include "amos_projection_search.h"

#include "../../include/amos_host_types.h"  // amos_proj_query

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

struct MotionArgs : ProjArgs {
    const amos_last_point *points;
    const MotionFrame *frames;
    amos_proj_query *query;
    uint8_t *projected;
    int *match;
    amos_motion_stats *stats;
    amos_best2 *best2;  // scratch, one per point
    int *accepted;      // scratch, one per point: -1, or bin << 16 | feature of the point's accepted match
    uint8_t *flags;     // scratch, one per point: bit 0 projected, bit 1 a projection that is not finite, bit 2 an octave outside the table
    int pass;  // 1: radius th; 2: radius th_retry, for the frames whose first search stayed below retry_below
};

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
    copy_desc(q.desc, lp.desc);
    int flags = 0;
    if (!(lp.flags & AMOS_LAST_POINT_SKIP)) {
        float xc, yc, zc;
        camera_point(c.Rcw, c.tcw, lp.pos, xc, yc, zc);
        const float invzc = (float)__ddiv_rn(1.0, (double)zc);
        if (!(invzc < 0)) {
            const float u = __fadd_rn(__fmul_rn(__fmul_rn(c.fx, xc), invzc), c.cx);
            const float v = __fadd_rn(__fmul_rn(__fmul_rn(c.fy, yc), invzc), c.cy);
            if (pixel_in_bounds(a, u, v, flags)) {
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
__device__ __forceinline__ WindowQuery load_motion_query(const MotionArgs &a, const MotionFrame &fr, int p)
{
    const amos_proj_query &q = a.query[p];
    WindowQuery o;
    o.u = q.u; o.v = q.v;
    o.ur = __fsub_rn(q.u, __fmul_rn(fr.cam.mbf, q.invz));  // :1665
    const int octave = q.octave;                           // inside the table: k_motion_project
    o.r = __fmul_rn(a.pass == 2 ? fr.cam.th_retry : fr.cam.th, a.scale[octave]);
    level_window(o, octave, fr.flags & 1, fr.flags & 2);
    o.d = load_desc_words(q.desc);
    return o;
}

// ---- the candidate loop of ORBmatcher.cc:1629-1690 against the empty frame (cell order x * 48 + y is the candidate order: the first
// candidate wins ties).  grid = (ceil(max points * 8 / 256), frames), block = 256.
__global__ __launch_bounds__(256) void k_motion_window_best2(const MotionArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    const MotionFrame &fr = a.frames[f];
    if (a.pass == 2 && a.stats[f].n_matches >= fr.cam.retry_below) return;  // the whole work-group: the first search stands
    const int p = fr.off0 + t / kWindowLanes;
    const bool active = p < fr.off1 && a.projected[p] != 0 && min(a.counts[f], a.capacity) > 0;
    WindowQuery q;
    if (active) q = load_motion_query(a, fr, p);
    lanes_window_best2(a, frame_view(a, f), q, active, t % kWindowLanes, kInitDist, [](int) { return true; }, p < fr.off1 ? a.best2 + p : nullptr);
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
    __shared__ TakenBitmap taken;
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
    const FrameView fv = frame_view(a, f);
    int *match = a.match + (size_t)f * cap;
    for (int w = lane; w < kTakenWords; w += 64) taken.w[w] = 0;
    if (lane < AMOS_HISTO_LENGTH) hist[lane] = 0;
    for (int i = lane; i < cap; i += 64) match[i] = -1;
    __syncthreads();
    int nProjected = 0, nMatches = 0, nResearched = 0, bad = 0;
    for (int base = off0; base < off1; base += 64) {
        const int p = base + lane;
        const bool valid = p < off1;
        const int fl = valid ? a.flags[p] : 0;
        bad |= fl & 6;
        amos_best2 rec = best2_from_keys(0xffffffffu, 0xffffffffu, nullptr, kInitDist);  // none
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
            if (taken.test(bi)) {
                if (si < 0) continue;  // the only candidate is taken
                if (!taken.test(si)) {
                    bi = si; bd = sd;
                } else {
                    nResearched++;
                    const amos_best2 r = wave_research(a, fv, load_motion_query(a, fr, base + k), taken, lane);
                    if (r.best_idx < 0) continue;
                    bi = r.best_idx; bd = r.best_dist;
                }
            }
            if (bd > AMOS_TH_HIGH) continue;
            nMatches++;
            int bin = 0;
            if (checkOri) bin = rotation_bin(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(angle), k)), fv.tk[bi].angle);  // :1683-1698
            if (lane == k) acc = (bin << 16) | bi;
            if (lane == 0) {
                match[bi] = base + k - off0;
                if (ho) taken.set(bi);
                if (checkOri) hist[bin]++;
            }
            __syncthreads();  // the bit is visible to every lane before the next point reads the bitmap
        }
        if (valid) a.accepted[p] = acc;
    }
    __threadfence_block();
    __syncthreads();  // lane 0's writes to match and hist are over before the pruning reads and overwrites
    if (checkOri) {
        int ind1, ind2, ind3;
        three_maxima(hist, ind1, ind2, ind3);
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

extern "C" {

int amos_match_motion_model_batch_device(amos_match *m, const amos_motion_search *s)
{
    int maxPoints;
    size_t total;
    int rc = check_point_search("amos_match_motion_model_batch_device", m, s, s && s->d_projected, &maxPoints, &total);
    if (rc != AMOS_OK) return rc;
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const PointScratch l = point_scratch(sizeof(MotionFrame) * (size_t)s->n_frames, total, true, 1);
    rc = grow(&m->dLocal, &m->capLocal, l.bytes);
    if (rc != AMOS_OK) return rc;
    std::vector<MotionFrame> frames((size_t)s->n_frames);
    bool retry = false;
    for (int f = 0; f < s->n_frames; f++) {
        MotionFrame &fr = frames[f];
        fr = MotionFrame{s->cameras[f], s->point_off[f], s->point_off[f + 1], 0};
        // :1584-1599.  twc = -Rcw^T tcw and tlc = Rlw twc + tlw are one gemm each: double accumulation, one rounding
        const amos_motion_camera &c = fr.cam;
        float twc[3];
        camera_centre(c.Rcw, c.tcw, twc);
        const float tlcZ = (float)((double)c.Rlw[6] * twc[0] + (double)c.Rlw[7] * twc[1] + (double)c.Rlw[8] * twc[2] + (double)c.tlw[2]);
        const bool bForward = tlcZ > c.mb && !c.mono, bBackward = -tlcZ > c.mb && !c.mono;
        fr.flags = (bForward ? 1 : 0) | (bBackward ? 2 : 0);
        retry = retry || c.retry_below > 0;
    }
    rc = upload_frames(m, frames.data(), sizeof(MotionFrame) * frames.size());
    if (rc != AMOS_OK) return rc;
    MotionArgs a;
    fill_proj_args(a, *s);
    a.points = s->d_points; a.frames = (const MotionFrame *)m->dLocal;
    a.query = s->d_query; a.projected = s->d_projected; a.match = s->d_match; a.stats = s->d_stats;
    a.best2 = (amos_best2 *)(m->dLocal + l.best2); a.accepted = (int *)(m->dLocal + l.accepted); a.flags = m->dLocal + l.flags;
    a.pass = 1;
    if (maxPoints > 0) hipLaunchKernelGGL(k_motion_project, dim3((maxPoints + 255) / 256, s->n_frames), dim3(256), 0, m->stream, a);
    for (int pass = 1; pass <= (retry ? 2 : 1); pass++) {
        a.pass = pass;
        if (maxPoints > 0) hipLaunchKernelGGL(k_motion_window_best2, window_grid(maxPoints, s->n_frames), dim3(256), 0, m->stream, a);
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
    const size_t np1 = (size_t)std::max(n_points, 1);
    return one_frame_search<amos_motion_search>(m, amos_match_motion_model_batch_device, kps_un, desc, u_right, n, n_points, np1 * sizeof(amos_last_point), scale_factors,
                                               n_levels, min_x, max_x, min_y, max_y, query, projected, match, stats,
                                               [&](amos_motion_search &s, uint8_t *d_flag, const uint8_t *zeros) {
        s.d_points = stage_input<amos_last_point>(m, n_points ? (const void *)points : zeros, sizeof(amos_last_point) * np1);
        s.cameras = camera;
        s.d_projected = d_flag;
    });
}

}  // extern "C"
