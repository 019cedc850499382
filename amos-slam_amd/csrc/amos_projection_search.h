// amos_projection_search.h -- what the projection-window searches share: k_window_best2 of amos_match.hip and the five map-point searches
// (local map: amos_local.hip, motion model: amos_motion.hip, relocalisation: amos_reloc.hip, Fuse: amos_fuse.hip, loop points:
// amos_loop_points.hip).  On the device:
//   - Frame::GetFeaturesInArea (Frame.cc:894-1003) plus the best / second-best Hamming loop over a frame's cell CSR (all six);
//   - the steps of a point's projection that they spell alike: camera_point, point_offset, normal_dot, in_distance_band, pixel_in_bounds,
//     copy_desc, predict_scale_level; keyframe_prefilter, the whole pre-filter of the two keyframe-side searches (Fuse, loop points);
//   - the parts of the greedy acceptance of local, motion, relocalisation and loop points: TakenBitmap, wave_research, rotation_bin,
//     three_maxima (Fuse has no greedy stage).  The sequential loop around them is written out in each accept kernel: three shared forms of it were
//     measured and each cost the relocalisation kernel 2 to 17 % (profiles/r14_point_searches.txt).
// On the host: the argument filling, validation, scratch layout and staging of their entries.
// A search itself keeps how it finds its query and which gates stand between the projection's steps, its extra filter and its accept loop.
#pragma once
#include "amos_match_core.h"
#include "amos_scene_flow.h"  // gemm_row

#include <climits>
#include <cmath>
#include <vector>

namespace amos {

constexpr int kInitDist = 256;  // bestDist / bestDist2 on entry of the reference's loops (ORBmatcher.cc:125-126, :1645-1646)

// what every search reads of its frames
struct ProjArgs {
    const amos_keypoint *kps;               // [frames][capacity]
    const uint8_t *desc;                    // [frames][capacity][32]
    const int *counts, *cellStart, *items;  // [frames], [frames][3073], [frames][capacity]
    const float *uRight;                    // [frames][capacity] or null: no right gate
    float scale[AMOS_MAX_LEVELS];
    float minX, maxX, minY, maxY, wInv, hInv;
    int capacity, nLevels;
};

// one frame of those arrays
struct FrameView { const int *cs, *it; const amos_keypoint *tk; const uint8_t *td; const float *tr; };
__device__ __forceinline__ FrameView frame_view(const ProjArgs &a, int f)
{
    const size_t o = (size_t)f * a.capacity;
    return FrameView{a.cellStart + (size_t)f * (kGridCells + 1), a.items + o, a.kps + o, a.desc + o * 32, a.uRight ? a.uRight + o : nullptr};
}

// what a search reads of one query
struct WindowQuery {
    float u, v, ur, r;  // r: the window's radius
    int lo, hi;         // the level window, inclusive
    Desc d;
};

// GetFeaturesInArea(u, v, r, minLevel, maxLevel) checks levels when minLevel > 0 || maxLevel >= 0 (Frame.cc:945).  Its three uses around
// an octave as inclusive windows: (octave, -1) forward, (0, octave) backward, (octave - 1, octave + 1) otherwise.
__device__ __forceinline__ void level_window(WindowQuery &q, int octave, bool forward, bool backward)
{
    if (forward) { q.lo = octave > 0 ? octave : INT_MIN; q.hi = INT_MAX; }
    else if (backward) { q.lo = 0; q.hi = octave; }
    else { q.lo = octave - 1; q.hi = octave + 1; }
}

// MapPoint::PredictScale (MapPoint.cc:571-586) without a library logarithm: the number of table entries below the ratio
// mfMaxDistance / dist, at most nLevels - 1 (a NaN ratio gives 0).  include/amos_frontend.h, "local map search", says where it differs
// from ceil(logf(ratio) / mfLogScaleFactor).
__device__ __forceinline__ int predict_scale_level(const ProjArgs &a, float maxDistance, float dist)
{
    const float ratio = __fdiv_rn(maxDistance, dist);
    int level = 0;
    for (int m = 0; m < a.nLevels; m++) level += ratio > a.scale[m] ? 1 : 0;
    return min(level, a.nLevels - 1);
}

// ---- the steps of a point's projection that the point searches (amos_local.hip, amos_motion.hip, amos_reloc.hip, amos_fuse.hip,
// amos_loop_points.hip) spell alike.  The gates between them, 1 / z and the order of the pixel's products differ on purpose between the
// frame searches, which keep them in their kernels, and the keyframe-side ones (keyframe_prefilter below); DESIGN.md section 1 lists them.

// Pc = R P + t: one gemm row each, double accumulation, one rounding
__device__ __forceinline__ void camera_point(const float *R, const float *t, const float *P, float &x, float &y, float &z)
{
    x = gemm_row(R, 0, P[0], P[1], P[2], t[0]);
    y = gemm_row(R, 1, P[0], P[1], P[2], t[1]);
    z = gemm_row(R, 2, P[0], P[1], P[2], t[2]);
}
// PO = P - Ow in float32 -> its length: the squares accumulated in double left to right, one square root, one rounding
__device__ __forceinline__ float point_offset(const float *P, const float *Ow, float PO[3])
{
    PO[0] = __fsub_rn(P[0], Ow[0]); PO[1] = __fsub_rn(P[1], Ow[1]); PO[2] = __fsub_rn(P[2], Ow[2]);
    const double n2 = __dadd_rn(__dadd_rn(__dmul_rn((double)PO[0], (double)PO[0]), __dmul_rn((double)PO[1], (double)PO[1])),
                                __dmul_rn((double)PO[2], (double)PO[2]));
    return (float)__dsqrt_rn(n2);
}
// PO . normal in double, left to right, not rounded to float
__device__ __forceinline__ double normal_dot(const float PO[3], const float *normal)
{
    return __dadd_rn(__dadd_rn(__dmul_rn((double)PO[0], (double)normal[0]), __dmul_rn((double)PO[1], (double)normal[1])),
                     __dmul_rn((double)PO[2], (double)normal[2]));
}
// the scale-invariance band of a map point's distance: strict on both sides, a NaN passes
__device__ __forceinline__ bool in_distance_band(float dist, float minD, float maxD) { return !(dist < __fmul_rn(0.8f, minD) || dist > __fmul_rn(1.2f, maxD)); }
// the frame searches' pixel gate: inside the inclusive bounds; a pixel that is not finite sets bit 1 of the point's flags instead
__device__ __forceinline__ bool pixel_in_bounds(const ProjArgs &a, float u, float v, int &flags)
{
    if (!(isfinite(u) && isfinite(v))) { flags |= 2; return false; }
    return !(u < a.minX || u > a.maxX) && !(v < a.minY || v > a.maxY);
}
// a point's descriptor into its query record, eight words
__device__ __forceinline__ void copy_desc(uint8_t *dst, const uint8_t *src)
{
#pragma unroll
    for (int k = 0; k < 8; k++) reinterpret_cast<uint32_t *>(dst)[k] = reinterpret_cast<const uint32_t *>(src)[k];
}

// The pre-filter of the keyframe-side searches (amos_fuse.hip: Fuse, ORBmatcher.cc:1042-1083 / :1199-1244; amos_loop_points.hip:
// SearchByProjection(pKF, Scw), :416-462) as include/amos_frontend.h "fuse search" defines it: p3Dc.z < 0 is out, invz = 1.0f / z,
// u = fx * (X * invz) + cx, the half-open KeyFrame::IsInImage (a pixel that is not finite fails it), the distance band, the 60-degree test
// in double, the predicted level.  -> 0 in view, or the gate that rejected the point; u, v and invz hold what was computed up to there.
enum { kViewBehind = 1, kViewImage = 2, kViewBand = 3, kViewAngle = 4 };
struct KeyframeProjection { float u, v, invz; int level; };
__device__ __forceinline__ int keyframe_prefilter(const ProjArgs &a, const float *Rcw, const float *tcw, const float *Ow, float fx, float fy, float cx,
                                                  float cy, const amos_map_point &mp, KeyframeProjection &o)
{
    o.u = o.v = o.invz = 0.f;
    o.level = 0;
    float PcX, PcY, PcZ;
    camera_point(Rcw, tcw, mp.pos, PcX, PcY, PcZ);
    if (PcZ < 0.0f) return kViewBehind;
    o.invz = __fdiv_rn(1.0f, PcZ);
    o.u = __fadd_rn(__fmul_rn(fx, __fmul_rn(PcX, o.invz)), cx);
    o.v = __fadd_rn(__fmul_rn(fy, __fmul_rn(PcY, o.invz)), cy);
    if (!(o.u >= a.minX && o.u < a.maxX && o.v >= a.minY && o.v < a.maxY)) return kViewImage;  // KeyFrame::IsInImage: a NaN or an infinity fails it
    float PO[3];
    const float dist = point_offset(mp.pos, Ow, PO);
    if (!in_distance_band(dist, mp.min_distance, mp.max_distance)) return kViewBand;
    if (normal_dot(PO, mp.normal) < __dmul_rn(0.5, (double)dist)) return kViewAngle;
    o.level = predict_scale_level(a, mp.max_distance, dist);
    return 0;
}

// one candidate of a window (CSR position j): its key dist << 16 | j, or none when a gate rejects it: the level window, the box, the right
// gate (ORBmatcher.cc:132-137, :1662-1669) and the loops' strict dist < initDist.  Occupancy and bitmap filters are the caller's.
__device__ __forceinline__ bool window_candidate(const WindowQuery &q, const FrameView &fv, int idx, int j, int initDist, unsigned &key)
{
    const amos_keypoint k = fv.tk[idx];
    if (k.octave < q.lo || k.octave > q.hi) return false;
    if (!(fabsf(__fsub_rn(k.x, q.u)) < q.r && fabsf(__fsub_rn(k.y, q.v)) < q.r)) return false;
    if (fv.tr) {
        const float tt = fv.tr[idx];
        if (tt > 0 && fabsf(__fsub_rn(q.ur, tt)) > q.r) return false;
    }
    const int d = hamming256(q.d, load_desc(fv.td + (size_t)idx * 32));
    key = ((unsigned)d << 16) | (unsigned)j;
    return d < initDist;  // (the last gate is no early return: the push behind it stays a select)
}

// keys dist << 16 | CSR position -> the record
__device__ __forceinline__ amos_best2 best2_from_keys(unsigned best, unsigned second, const int *it, int noneDist)
{
    amos_best2 r;
    r.best_idx = best == 0xffffffffu ? -1 : it[best & 0xffffu];
    r.best_dist = best == 0xffffffffu ? noneDist : (int)(best >> 16);
    r.second_idx = second == 0xffffffffu ? -1 : it[second & 0xffffu];
    r.second_dist = second == 0xffffffffu ? noneDist : (int)(second >> 16);
    return r;
}

// The prepass of a search: kWindowLanes lanes per query, lane `sub` of them walks every kWindowLanes-th grid column of the window.  The
// reference walks the cells x-major, then y, then insertion order = ascending CSR position, and its strict-< updates keep the FIRST of
// equal distances: a min-reduction over keys (dist << 16 | CSR position) gives the same best two whatever the evaluation order.  All lanes
// of a group call it; q is read only where `active`, the group's first lane writes *out (if not null); keep(idx) is the search's own filter.
// lanes_window_keys leaves the two keys in every lane of the group (amos_fuse.hip and amos_sim3_search.hip keep no record in memory).
template <class Keep>
__device__ __forceinline__ void lanes_window_keys(const ProjArgs &a, const FrameView &fv, const WindowQuery &q, bool active, int sub, int initDist,
                                                  Keep keep, unsigned &best, unsigned &second)
{
    CellRange c;
    c.x0 = 0; c.x1 = -1; c.y0 = c.y1 = 0;  // idle lanes walk no column and keep the group shuffles convergent
    if (active) c = cell_range(q.u, q.v, q.r, a.minX, a.minY, a.wInv, a.hInv);
    best = second = 0xffffffffu;
    for (int ix = c.x0 + sub; ix <= c.x1; ix += kWindowLanes) {
        int b, e;  // cells (ix, y0..y1) are consecutive in the CSR: one item range per column
        column_items(fv.cs, c, ix, b, e);
        for (int j = b; j < e; j++) {
            const int idx = fv.it[j];
            unsigned key;
            if (keep(idx) && window_candidate(q, fv, idx, j, initDist, key)) top2_push(best, second, key);
        }
    }
#pragma unroll
    for (int off = kWindowLanes / 2; off > 0; off >>= 1) {
        const unsigned ob = __shfl_xor(best, off, kWindowLanes), os = __shfl_xor(second, off, kWindowLanes);
        top2_merge(best, second, ob, os);
    }
}
template <class Keep>
__device__ __forceinline__ void lanes_window_best2(const ProjArgs &a, const FrameView &fv, const WindowQuery &q, bool active, int sub, int initDist,
                                                   Keep keep, amos_best2 *out)
{
    unsigned best, second;
    lanes_window_keys(a, fv, q, active, sub, initDist, keep, best, second);
    if (out && sub == 0) *out = best2_from_keys(best, second, fv.it, initDist);
}

constexpr int kTakenWords = 65536 / 32;  // the features a greedy loop has taken, one bit each, in LDS (capacity <= 65536)
struct TakenBitmap {
    uint32_t w[kTakenWords];
    __device__ __forceinline__ bool test(int i) const { return (w[i >> 5] >> (i & 31)) & 1u; }
    // feature i, or feature j >= 0, is taken: both words are read before either is looked at, one LDS round trip in a sequential loop
    __device__ __forceinline__ bool either(int i, int j) const { const uint32_t a = w[i >> 5], b = w[max(j, 0) >> 5]; return ((a >> (i & 31)) | (j >= 0 ? b >> (j & 31) : 0u)) & 1u; }
    __device__ __forceinline__ void set(int i) { w[i >> 5] |= 1u << (i & 31); }
};

// The rotation histogram of a greedy loop.  The bin of an accepted match (ORBmatcher.cc:314-323, :1683-1698): float32, every operation
// rounded in source order.  (The reference asserts the range; an angle that is not finite lands in bin 0.)
__device__ __forceinline__ int rotation_bin(float angle1, float angle2)
{
    float rot = __fsub_rn(angle1, angle2);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, AMOS_HISTO_LENGTH / 360.0f));
    if (bin == AMOS_HISTO_LENGTH) bin = 0;
    return min(max(bin, 0), AMOS_HISTO_LENGTH - 1);
}
// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1866-1908) over the bins' counts: strict comparisons, the earlier bin wins a tie; -1: none
__device__ __forceinline__ void three_maxima(const int *hist, int &ind1, int &ind2, int &ind3)
{
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;  // (locals, not the references: those would be kept in memory)
    for (int i = 0; i < AMOS_HISTO_LENGTH; i++) {
        const int s = hist[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            i3 = i2; i2 = i1; i1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            i3 = i2; i2 = i;
        } else if (s > max3) {
            max3 = s; i3 = i;
        }
    }
    if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { i2 = -1; i3 = -1; }
    else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) i3 = -1;
    ind1 = i1; ind2 = i2; ind3 = i3;
}

// the whole wave searches a query's window again, against the bitmap; the record comes back wave-uniform
__device__ __forceinline__ amos_best2 wave_research(const ProjArgs &a, const FrameView &fv, const WindowQuery &q, const TakenBitmap &taken, int lane)
{
    const CellRange c = cell_range(q.u, q.v, q.r, a.minX, a.minY, a.wInv, a.hInv);
    unsigned best, second;
    wave_window_best2(fv.cs, fv.it, c, lane, [&](int idx, int j, unsigned &key) {
        return !taken.test(idx) && window_candidate(q, fv, idx, j, kInitDist, key);
    }, best, second);
    return best2_from_keys(best, second, fv.it, kInitDist);
}

// ---------------------------------------------------------------------------------------------------------------- host

inline size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

// S: amos_window_search, amos_local_search, amos_motion_search, or amos_reloc_search (which has no right coordinates: uRight = null)
template <class S>
inline void fill_proj_args(ProjArgs &a, const S &s, const float *uRight)
{
    a.kps = s.d_kps; a.desc = s.d_desc; a.counts = s.d_counts; a.cellStart = s.d_cell_start; a.items = s.d_items; a.uRight = uRight;
    for (int l = 0; l < AMOS_MAX_LEVELS; l++) a.scale[l] = l < s.n_levels ? s.scale_factors[l] : 0.f;
    a.minX = s.min_x; a.maxX = s.max_x; a.minY = s.min_y; a.maxY = s.max_y;
    a.wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(s.max_x - s.min_x);  // Frame.cc:302-303
    a.hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(s.max_y - s.min_y);
    a.capacity = s.capacity; a.nLevels = s.n_levels;
}
template <class S>
inline void fill_proj_args(ProjArgs &a, const S &s) { fill_proj_args(a, s, s.d_u_right); }

// What the batch entries of the point searches check alike (own: the entry's own pointers and counts are there).  The point ranges are one
// per frame, or one per pair (nGroups = &S::n_pairs) with frameOf naming each pair's frame.  -> the most points of a range, of all
template <class S>
inline int check_point_search(const char *name, const amos_match *m, const S *s, bool own, int *maxPoints, size_t *total,
                              int32_t S::*nGroups = &S::n_frames, const int32_t *S::*frameOf = nullptr)
{
    if (!m || !s || !own || !s->d_kps || !s->d_desc || !s->d_counts || !s->d_cell_start || !s->d_items || !s->d_points || !s->point_off ||
        !s->cameras || !s->scale_factors || !s->d_query || !s->d_match || !s->d_stats || s->n_frames < 1 || s->capacity < 1 ||
        s->capacity > 65536 || s->n_levels < 1 || s->n_levels > AMOS_MAX_LEVELS || !(s->max_x > s->min_x) || !(s->max_y > s->min_y)) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    *maxPoints = 0;
    if (s->point_off[0] < 0) { set_error("%s: point_off[0] < 0", name); return AMOS_ERR_INVALID; }
    const int groups = s->*nGroups;
    for (int g = 0; g < groups; g++) {
        if (frameOf && ((s->*frameOf)[g] < 0 || (s->*frameOf)[g] >= s->n_frames)) { set_error("%s: frame_of_pair[%d] outside the frames", name, g); return AMOS_ERR_INVALID; }
        if (s->point_off[g + 1] < s->point_off[g]) { set_error("%s: point_off descends at %d", name, g); return AMOS_ERR_INVALID; }
        *maxPoints = std::max(*maxPoints, s->point_off[g + 1] - s->point_off[g]);
    }
    *total = (size_t)s->point_off[groups];
    return AMOS_OK;
}

// The per-call scratch of a point search in dLocal: the frame (or pair) records that upload_frames writes, one amos_best2 per point, then
// as the search asks one int per point (`accepted`) and one or two planes of one byte per point (flags), each aligned to 64 bytes
struct PointScratch { size_t best2, accepted, flags, flags2, bytes; };
inline PointScratch point_scratch(size_t recordBytes, size_t total, bool accepted, int flagPlanes)
{
    const size_t best2 = align64(recordBytes), acc = best2 + align64(sizeof(amos_best2) * total), flags = acc + (accepted ? align64(sizeof(int) * total) : 0);
    return PointScratch{best2, acc, flags, flags + align64(total), flags + (size_t)flagPlanes * align64(total)};
}

// -Rcw^T tcw (the motion-model search's twc, the relocalisation search's Ow): double accumulation left to right, one rounding
inline void camera_centre(const float *Rcw, const float *tcw, float *out)
{
    for (int k = 0; k < 3; k++) out[k] = (float)-(((double)Rcw[k] * tcw[0] + (double)Rcw[3 + k] * tcw[1]) + (double)Rcw[6 + k] * tcw[2]);
}

// Frame::PosInGrid (Frame.cc:1007-1030) -> the cell x * rows + y, or -1 outside the grid
inline int32_t pos_in_grid(float x, float y, float min_x, float min_y, float wInv, float hInv)
{
    const int px = (int)roundf((x - min_x) * wInv), py = (int)roundf((y - min_y) * hInv);
    return px >= 0 && px < AMOS_FRAME_GRID_COLS && py >= 0 && py < AMOS_FRAME_GRID_ROWS ? px * AMOS_FRAME_GRID_ROWS + py : -1;
}

// the launch grid of a prepass: kWindowLanes lanes per point, 256 threads per block, one row of blocks per frame or pair
inline dim3 window_grid(int maxPoints, int groups) { return dim3((unsigned)(((size_t)maxPoints * kWindowLanes + 255) / 256), groups); }

// The per-frame parameters of a call to the front of dLocal, through the handle's own pinned buffer: the previous call's copy out of it
// has to be over before it is written again (an event, not a stream synchronisation: the kernels behind that copy are not waited for).
inline int upload_frames(amos_match *m, const void *frames, size_t bytes)
{
    if (!m->localCopied) AMOS_HIP_CHECK(hipEventCreateWithFlags(&m->localCopied, hipEventDisableTiming));
    else AMOS_HIP_CHECK(hipEventSynchronize(m->localCopied));
    if (bytes > m->capHLocal) {
        if (m->hLocal) (void)hipHostFree(m->hLocal);
        m->hLocal = nullptr;
        m->capHLocal = 0;
        const size_t n = std::max<size_t>(2 * bytes, 4096);
        AMOS_HIP_CHECK(hipHostMalloc((void **)&m->hLocal, n, hipHostMallocDefault));
        m->capHLocal = n;
    }
    std::memcpy(m->hLocal, frames, bytes);
    AMOS_HIP_CHECK(hipMemcpyAsync(m->dLocal, m->hLocal, bytes, hipMemcpyHostToDevice, m->stream));
    AMOS_HIP_CHECK(hipEventRecord(m->localCopied, m->stream));
    return AMOS_OK;
}

// The one-frame host forms of the point searches (S: amos_local_search, amos_motion_search, amos_reloc_search): ONE frame of n features and n_points points,
// host arrays in and out.  Lays out the result buffer (query records, one byte per point, match, stats: the download; then the grid),
// computes Frame::PosInGrid, stages the frame's arrays and fills the fields of S that both kinds have; own(s, d_flag, zeros) stages the entry's
// own inputs (ownBytes of them) and fills its own fields; then one upload, AssignFeaturesToGrid, the batch form, one download, the copy-out.
// match_in (amos_reloc_search: d_match is read too): `match` travels up with the inputs and is copied into the result buffer first.
// (amos_reloc_search has no d_u_right and counts pairs beside frames: the two setters below are what differs in its layout)
template <class S>
inline auto set_u_right(S &s, const float *p) -> decltype((void)s.d_u_right) { s.d_u_right = p; }
inline void set_u_right(amos_reloc_search &, const float *) {}
template <class S>
inline auto set_n_frames(S &s, int) -> decltype((void)s.n_pairs) { s.n_frames = 1; s.n_pairs = 1; }
template <class S>
inline void set_n_frames(S &s, long) { s.n_frames = 1; }
template <class S, class Own>
inline int one_frame_search(amos_match *m, int (*batch)(amos_match *, const S *), const amos_keypoint *kps_un, const uint8_t *desc,
                            const float *u_right, int n, int n_points, size_t ownBytes, const float *scale_factors, int n_levels, float min_x,
                            float max_x, float min_y, float max_y, void *query, uint8_t *flag, int32_t *match, void *stats, Own own, bool match_in = false)
{
    S s;
    const size_t querySize = sizeof(*s.d_query), statsSize = sizeof(*s.d_stats);
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const int cap = std::max(n, 1);
    const size_t np = (size_t)n_points, np1 = std::max<size_t>(np, 1);
    const size_t oFlag = align64(querySize * np1), oMatch = oFlag + align64(np1), oStats = oMatch + align64(sizeof(int32_t) * (size_t)cap),
                 oEnd = oStats + align64(statsSize), oItems = oEnd + align64(sizeof(int32_t) * (kGridCells + 1)),
                 oAll = oItems + align64(sizeof(int32_t) * (size_t)cap);
    int rc = stage_begin(m, (size_t)cap * (sizeof(amos_keypoint) + 32 + 4 + 4) + 64 + ownBytes + oEnd + (match_in ? align64(sizeof(int32_t) * (size_t)cap) : 0));
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, oAll);
    if (rc != AMOS_OK) return rc;
    const float wInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(max_x - min_x);
    const float hInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(max_y - min_y);
    std::vector<int32_t> cell((size_t)cap, -1);
    for (int i = 0; i < n; i++) cell[i] = pos_in_grid(kps_un[i].x, kps_un[i].y, min_x, min_y, wInv, hInv);
    const std::vector<uint8_t> zeros(std::max<size_t>((size_t)cap * 32, 256), 0);  // a frame without features or points still hands valid arrays down
    const int32_t count = n, off[2] = {0, n_points};
    uint8_t *out = (uint8_t *)m->dOut;
    s.d_kps = stage_input<amos_keypoint>(m, n ? (const void *)kps_un : zeros.data(), sizeof(amos_keypoint) * (size_t)cap);
    s.d_desc = stage_input<uint8_t>(m, n ? desc : zeros.data(), (size_t)cap * 32);
    set_u_right(s, u_right && n ? stage_input<float>(m, u_right, sizeof(float) * (size_t)cap) : nullptr);
    const int32_t freeFeature = -1;  // (cap is 1 when n is 0)
    const int32_t *dMatchIn = match_in ? stage_input<int32_t>(m, n ? match : &freeFeature, sizeof(int32_t) * (size_t)cap) : nullptr;
    const int32_t *dCell = stage_input<int32_t>(m, cell.data(), sizeof(int32_t) * (size_t)cap);
    s.d_counts = stage_input<int32_t>(m, &count, sizeof(count));
    s.d_cell_start = (int32_t *)(out + oEnd); s.d_items = (int32_t *)(out + oItems);
    s.point_off = off; s.scale_factors = scale_factors;
    s.d_query = (decltype(s.d_query))out; s.d_match = (int32_t *)(out + oMatch); s.d_stats = (decltype(s.d_stats))(out + oStats);
    set_n_frames(s, 0);
    s.capacity = cap; s.n_levels = n_levels;
    s.min_x = min_x; s.max_x = max_x; s.min_y = min_y; s.max_y = max_y;
    own(s, out + oFlag, zeros.data());
    int32_t *dStart = (int32_t *)(out + oEnd), *dItems = (int32_t *)(out + oItems);
    if ((rc = stage_flush(m)) != AMOS_OK) return rc;
    if (dMatchIn) AMOS_HIP_CHECK(hipMemcpyAsync(out + oMatch, dMatchIn, sizeof(int32_t) * (size_t)cap, hipMemcpyDeviceToDevice, m->stream));
    if ((rc = amos_frame_grid_build_batch_device(m, dCell, s.d_counts, 1, cap, dStart, dItems)) != AMOS_OK ||
        (rc = batch(m, &s)) != AMOS_OK) return rc;
    const uint8_t *h = m->hStage + stage_take(m, oEnd);
    AMOS_HIP_CHECK(hipMemcpyAsync((void *)h, out, oEnd, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (np) {
        std::memcpy(query, h, querySize * np);
        std::memcpy(flag, h + oFlag, np);
    }
    if (n) std::memcpy(match, h + oMatch, sizeof(int32_t) * (size_t)n);
    std::memcpy(stats, h + oStats, statsSize);
    return AMOS_OK;
}

}  // namespace amos
