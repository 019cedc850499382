// amos_new_points.hip -- LocalMapping::CreateNewMapPoints between its search and its `new MapPoint` (LocalMapping.cc:424-597) for the pairs
// of ONE amos_match_triangulation_batch_device call, reading d_match12 where the search left it.  The semantics (verdicts, the claim rule,
// what a disabled pair writes) are defined in include/amos_frontend.h, "new map points"; the arithmetic is amos_new_points_core.h.
//
// Two launches on the matcher's stream.  k_new_points_solve: grid = (chunks of 256 keyframe-1 features) x pairs; a work-group compacts
// the matched features of its chunk (block_compact) so that the lanes that run triangulate_match -- the 4 x 4 Jacobi among it -- are dense
// (matches are 10-25 % of the features), one match per lane; verdict and x3D go to per-feature scratch rows.  k_new_points_emit: one
// work-group per pair applies the claim rule by scanning the scratch rows of the earlier pairs with the same keyframe-1 slot, compacts
// the accepted matches in ascending idx1 and sums the stats.  No atomics; every barrier, ballot and shuffle is reached by whole
// work-groups (the only early return is on values that are uniform over the work-group).
#include "amos_block.h"
#include "amos_match_core.h"
#include "amos_projection_search.h"
#include "amos_new_points_core.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace amos {

static_assert(sizeof(amos_kf_camera) == 96, "amos_kf_camera is 96 bytes (include/amos_frontend.h)");
static_assert(sizeof(amos_new_point) == 24 && sizeof(amos_new_points_stats) == 64, "amos_new_point is 24 bytes, amos_new_points_stats 64");

constexpr int kNewPtThreads = 256;
constexpr int kNewPtBadMatch = -2;  // scratch verdict of a match12 entry outside keyframe 2

struct NewPtArgs {
    const amos_keypoint *kps, *kpsRaw;
    const int *counts;
    const float *uRight, *depth;
    const int *pairs1, *pairs2;
    const int *match;
    const float *scale, *sigma2;
    const amos_kf_camera *cameras;  // scratch: [nFrames]
    const int *enabled;             // scratch: [nPairs]
    int *verdict;                   // scratch: [nPairs][capacity], written by k_new_points_solve for every feature of a pair that runs
    float *x3d;                     // scratch: [nPairs][capacity][3], written for the matches
    amos_new_point *outNew;
    int *outVerdict;
    amos_new_points_stats *stats;
    int nFrames, nPairs, capacity, nLevels;
};

// the pair takes part: enabled, both slots inside the frames.  Uniform over a work-group.
__device__ __forceinline__ bool new_pt_runs(const NewPtArgs &a, int p)
{
    return a.enabled[p] && (unsigned)a.pairs1[p] < (unsigned)a.nFrames && (unsigned)a.pairs2[p] < (unsigned)a.nFrames;
}

__device__ __forceinline__ newpt::Feature new_pt_feature(const NewPtArgs &a, int slot, int idx)
{
    const size_t o = (size_t)slot * a.capacity + idx;
    const amos_keypoint kp = a.kps[o];
    newpt::Feature f;
    f.x = kp.x; f.y = kp.y; f.octave = kp.octave;
    f.rawX = a.kpsRaw[o].x; f.rawY = a.kpsRaw[o].y;
    f.uRight = a.uRight ? a.uRight[o] : -1.0f;
    f.depth = f.uRight >= 0 ? a.depth[o] : -1.0f;  // (read only for a stereo feature)
    return f;
}

__global__ __launch_bounds__(kNewPtThreads) void k_new_points_solve(const NewPtArgs a)
{
    __shared__ int sWave[kNewPtThreads / 64];
    __shared__ int sList[kNewPtThreads];
    const int p = blockIdx.y, base = blockIdx.x * kNewPtThreads, t = threadIdx.x;
    if (!new_pt_runs(a, p)) return;
    const int cap = a.capacity, slot1 = a.pairs1[p], slot2 = a.pairs2[p];
    const int n1 = min(max(a.counts[slot1], 0), cap), n2 = min(max(a.counts[slot2], 0), cap);
    const int *match = a.match + (size_t)p * cap;
    int *verdict = a.verdict + (size_t)p * cap;
    int none = -1;  // what this lane's feature gets when it holds no match
    const int total = block_compact<kNewPtThreads>(min(kNewPtThreads, cap - base), sWave,
        [&](int i) {
            const int m = base + i < n1 ? match[base + i] : -1;
            none = m == -1 ? -1 : kNewPtBadMatch;
            return (unsigned)m < (unsigned)n2;
        },
        [&](int i, int c) {
            if (c >= 0) sList[c] = i;
            else verdict[base + i] = none;
        });
    if (t >= total) return;  // (no barrier follows)
    const int idx1 = base + sList[t], idx2 = match[idx1];
    const newpt::Feature f1 = new_pt_feature(a, slot1, idx1), f2 = new_pt_feature(a, slot2, idx2);
    float x3D[3];
    verdict[idx1] = newpt::triangulate_match(a.cameras[slot1], a.cameras[slot2], f1, f2, a.scale, a.sigma2, a.nLevels, x3D);
    float *out = a.x3d + ((size_t)p * cap + idx1) * 3;
    out[0] = x3D[0]; out[1] = x3D[1]; out[2] = x3D[2];
}

__global__ __launch_bounds__(kNewPtThreads) void k_new_points_emit(const NewPtArgs a)
{
    __shared__ int sWave[kNewPtThreads / 64];
    const int p = blockIdx.x, t = threadIdx.x, cap = a.capacity;
    int *outVerdict = a.outVerdict ? a.outVerdict + (size_t)p * cap : nullptr;
    if (!new_pt_runs(a, p)) {
        if (outVerdict)
            for (int i = t; i < cap; i += kNewPtThreads) outVerdict[i] = -1;
        if (t == 0) {
            amos_new_points_stats s = {};
            s.status = a.enabled[p] ? AMOS_NEW_POINTS_BAD_SLOT : 0;
            a.stats[p] = s;
        }
        return;
    }
    const int slot1 = a.pairs1[p];
    const int *match = a.match + (size_t)p * cap;
    const int *verdict = a.verdict + (size_t)p * cap;
    const float *x3d = a.x3d + (size_t)p * cap * 3;
    amos_new_point *outNew = a.outNew + (size_t)p * cap;
    int count[AMOS_NEW_POINT_VERDICTS] = {};
    int bad = 0, v = -1;
    const int nNew = block_compact<kNewPtThreads>(cap, sWave,
        [&](int i) {
            v = verdict[i];
            if (v == kNewPtBadMatch) { bad = 1; v = -1; }
            if ((unsigned)v <= (unsigned)AMOS_NEW_POINT_UNPROJECTED_2) {
                for (int q = 0; q < p; q++)  // the claim rule: an earlier pair of the same keyframe 1 accepted this feature's match
                    if (a.pairs1[q] == slot1 && new_pt_runs(a, q) && (unsigned)a.verdict[(size_t)q * cap + i] <= (unsigned)AMOS_NEW_POINT_UNPROJECTED_2) {
                        v = AMOS_NEW_POINT_CLAIMED;
                        break;
                    }
            }
            return (unsigned)v <= (unsigned)AMOS_NEW_POINT_UNPROJECTED_2;
        },
        [&](int i, int c) {
            if (outVerdict) outVerdict[i] = v;
#pragma unroll
            for (int k = 0; k < AMOS_NEW_POINT_VERDICTS; k++) count[k] += v == k ? 1 : 0;
            if (c >= 0) {
                amos_new_point r;
                r.idx1 = i; r.idx2 = match[i];
                r.x = x3d[3 * i]; r.y = x3d[3 * i + 1]; r.z = x3d[3 * i + 2];
                r.verdict = v;
                outNew[c] = r;
            }
        });
    amos_new_points_stats s = {};
#pragma unroll
    for (int k = 0; k < AMOS_NEW_POINT_VERDICTS; k++) {
        s.n_verdict[k] = block_sum<kNewPtThreads>(count[k], sWave);
        s.n_matches += s.n_verdict[k];
    }
    bad = block_sum<kNewPtThreads>(bad, sWave);
    s.n_new = nNew;
    s.status = (bad ? AMOS_NEW_POINTS_BAD_MATCH : 0) | (s.n_verdict[AMOS_NEW_POINT_OCTAVE] ? AMOS_NEW_POINTS_BAD_OCTAVE : 0);
    if (t == 0) a.stats[p] = s;
}

static bool new_pt_camera_ok(const amos_kf_camera &c)
{
    const float *f = c.Rcw;  // the record is 24 floats
    for (int i = 0; i < 24; i++)
        if (!std::isfinite(f[i])) return false;
    return c.fx > 0 && c.fy > 0;
}

}  // namespace amos

using namespace amos;

extern "C" {

int amos_kf_geometry_from_poses(const amos_kf_camera *c1, const amos_kf_camera *c2, amos_kf_geometry *g)
{
    if (!c1 || !c2 || !g) {
        set_error("amos_kf_geometry_from_poses: invalid argument");
        return AMOS_ERR_INVALID;
    }
    return newpt::pair_geometry(*c1, *c2, g) ? 1 : 0;
}

int amos_match_new_points_batch_device(amos_match *m, const amos_new_points *s)
{
    static const char *name = "amos_match_new_points_batch_device";
    if (!m || !s || !s->d_kps || !s->d_counts || (s->d_u_right && !s->d_depth) || !s->d_pairs_1 || !s->d_pairs_2 || !s->d_match12 ||
        !s->d_scale_factors || !s->d_level_sigma2 || !s->cameras || !s->pairs_1 || !s->pairs_2 || !s->d_new || !s->d_stats || s->n_frames < 1 ||
        s->n_pairs < 1 || s->n_pairs > AMOS_NEW_POINTS_MAX_PAIRS || s->capacity < 1 || s->capacity > 65536 || s->n_levels < 1 ||
        s->n_levels > AMOS_MAX_LEVELS) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    const int np = s->n_pairs;
    for (int k = 0; k < np; k++) {
        if ((unsigned)s->pairs_1[k] >= (unsigned)s->n_frames || (unsigned)s->pairs_2[k] >= (unsigned)s->n_frames) {
            set_error("%s: pair %d names a frame slot outside [0, %d)", name, k, s->n_frames);
            return AMOS_ERR_INVALID;
        }
        if (s->enabled && !s->enabled[k]) continue;
        for (int j = 0; j < k; j++)
            if ((!s->enabled || s->enabled[j]) && s->pairs_2[j] == s->pairs_2[k]) {
                set_error("%s: pairs %d and %d share keyframe-2 slot %d", name, j, k, s->pairs_2[k]);
                return AMOS_ERR_INVALID;
            }
        if (!new_pt_camera_ok(s->cameras[s->pairs_1[k]]) || !new_pt_camera_ok(s->cameras[s->pairs_2[k]])) {
            set_error("%s: pair %d: a camera is not finite or has fx, fy <= 0", name, k);
            return AMOS_ERR_INVALID;
        }
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    // the call's scratch: the cameras and the enabled flags (uploaded), then the verdict and x3D rows
    const size_t plane = (size_t)np * (size_t)s->capacity;
    const size_t bytesCams = align64(sizeof(amos_kf_camera) * (size_t)s->n_frames), bytesEnabled = align64(sizeof(int) * (size_t)np),
                 bytesVerdict = align64(sizeof(int) * plane), bytesX3d = align64(sizeof(float) * 3 * plane);
    int rc = grow(&m->dLocal, &m->capLocal, bytesCams + bytesEnabled + bytesVerdict + bytesX3d);
    if (rc != AMOS_OK) return rc;
    std::vector<uint8_t> host(bytesCams + bytesEnabled, 0);
    std::memcpy(host.data(), s->cameras, sizeof(amos_kf_camera) * (size_t)s->n_frames);
    int *en = (int *)(host.data() + bytesCams);
    for (int k = 0; k < np; k++) en[k] = !s->enabled || s->enabled[k] ? 1 : 0;
    rc = upload_frames(m, host.data(), host.size());
    if (rc != AMOS_OK) return rc;
    NewPtArgs a;
    a.kps = s->d_kps; a.kpsRaw = s->d_kps_raw ? s->d_kps_raw : s->d_kps; a.counts = s->d_counts; a.uRight = s->d_u_right; a.depth = s->d_depth;
    a.pairs1 = s->d_pairs_1; a.pairs2 = s->d_pairs_2; a.match = s->d_match12; a.scale = s->d_scale_factors; a.sigma2 = s->d_level_sigma2;
    a.cameras = (const amos_kf_camera *)m->dLocal; a.enabled = (const int *)(m->dLocal + bytesCams);
    a.verdict = (int *)(m->dLocal + bytesCams + bytesEnabled); a.x3d = (float *)(m->dLocal + bytesCams + bytesEnabled + bytesVerdict);
    a.outNew = s->d_new; a.outVerdict = s->d_verdict; a.stats = s->d_stats;
    a.nFrames = s->n_frames; a.nPairs = np; a.capacity = s->capacity; a.nLevels = s->n_levels;
    hipLaunchKernelGGL(k_new_points_solve, dim3((s->capacity + kNewPtThreads - 1) / kNewPtThreads, np), dim3(kNewPtThreads), 0, m->stream, a);
    hipLaunchKernelGGL(k_new_points_emit, dim3(np), dim3(kNewPtThreads), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

}  // extern "C"
