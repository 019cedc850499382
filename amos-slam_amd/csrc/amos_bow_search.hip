// amos_bow_search.hip -- the three greedy searches over a pair of FeatureVectors (the CSR of amos_bow_transform_batch_device, amos_bow.hip),
// for a batch of (side 1, side 2) pairs of resident frames: ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:230-382: side 1
// is the keyframe, side 2 the frame), ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (:656-799) and ORBmatcher::SearchForTriangulation
// (:810-1009).
//
// All are the same two launches on the matcher's stream, built from one prepass and one acceptance template over a policy (the query
// filter, the candidate filter, the key order, what a taken record means, the distance bound and the ratio test, which side indexes the result):
// k_list_best2 (eight lanes per list position of side 1: the best two side-2 features of its node under the filters that do not depend on
// what has been matched) and k_list_accept (one wave per pair: the reference's sequential loop over those records with the taken side-2
// features as a bitmap in LDS, then the rotation histogram's pruning).  The semantics are defined in include/amos_frontend.h, "bag of words".
#include "amos_bow_list.h"

#include <vector>

namespace amos {

static_assert(sizeof(amos_bow_search_stats) == 16, "amos_bow_search_stats is 16 bytes (include/amos_frontend.h)");

struct ListSearchArgs {
    const amos_keypoint *kps;
    const uint8_t *desc;
    const int *counts, *nNodes;
    const uint32_t *nodeIds;
    const int *nodeOff, *nodeIdx;
    const uint8_t *hasPoint;
    const float *uRight;
    const int *pairs1, *pairs2;
    int *match;  // per pair: indexed by side 1's feature and holding side 2's, or the other way round (the policy's kMatchBySide2)
    amos_bow_search_stats *stats;
    amos_best2 *best2;  // scratch, per pair and side-1 list position: the prepass record (indices are side-2 features)
    int *part;          // scratch, alike: -1: no query, -2: a feature index outside side 1, else side 2's node (its place in the node list)
                        // in the low 20 bits and kPartBadOctave when a candidate's octave was out of range
    int *accepted;      // scratch, alike: -1, or the bin of the query's accepted match (under kMatchBySide2: bin << 16 | side-2 feature, the
                        // entry of `match` it wrote; otherwise that entry is the query's own feature)
    const amos_kf_geometry *geometry;  // triangulation: [pairs]
    const float *scale, *sigma2;       // triangulation: [nLevels]
    int capacity, nLevels;
    float nnRatio;
    int checkOri, onlyStereo;
};
constexpr int kPartNodeMask = 0xfffff, kPartBadOctave = 1 << 20;  // (a node's place is below 65536)

// what the acceptance does with a prepass record
enum Taken { kKeep, kSecond, kAgain, kNone };

// ---- SearchByBoW(pKF, F, vpMapPointMatches): side 1 is the keyframe, side 2 the frame
struct BowFramePolicy {
    struct Query {};
    static constexpr bool kMatchBySide2 = true;  // match[frame feature] = keyframe feature
    // :264-270: only the keyframe's features need a good map point
    __device__ static bool query_ok(const ListSearchArgs &a, int slot1, int idx1) { return !a.hasPoint || a.hasPoint[(size_t)slot1 * a.capacity + idx1]; }
    __device__ static Query query(const ListSearchArgs &, int, const BowSide &, int, int) { return Query{}; }
    // :278-304 without the "already matched" test: dist < 256 (bestDist1's start); the frame's has_point is never read
    __device__ static bool candidate(const ListSearchArgs &, const Query &, const Desc &q, const BowSide &s2, int, int idx2, int &dist, int &)
    {
        dist = hamming256(q, load_desc(s2.desc + (size_t)idx2 * 32));
        return dist < kInitDist;
    }
    // the first of equal distances
    __device__ static unsigned key(int dist, int pos) { return ((unsigned)dist << 16) | (unsigned)pos; }
    __device__ static int pos(unsigned key) { return (int)(key & 0xffffu); }
    // the second best distance enters the ratio test: the record stands only when neither of its two is taken
    __device__ static Taken taken(const TakenBitmap &t, int bi, int si) { return t.either(bi, si) ? kAgain : kKeep; }
    // :306-309: bestDist1 <= TH_LOW, then the ratio test
    static constexpr int kMaxDist = AMOS_TH_LOW;
    __device__ static bool ratio_ok(const ListSearchArgs &a, int bd, int sd) { return (float)bd < __fmul_rn(a.nnRatio, (float)sd); }
};

// ---- SearchByBoW(pKF1, pKF2, vpMatches12): the search above between two keyframes, but for
struct BowKfPolicy : BowFramePolicy {
    static constexpr bool kMatchBySide2 = false;  // match12[idx1] = idx2
    // :700-722 without the vbMatched2 test: keyframe 2's feature needs a good map point too
    __device__ static bool candidate(const ListSearchArgs &a, const Query &pq, const Desc &q, const BowSide &k2, int slot2, int idx2, int &dist, int &bad)
    {
        if (a.hasPoint && !a.hasPoint[(size_t)slot2 * a.capacity + idx2]) return false;
        return BowFramePolicy::candidate(a, pq, q, k2, slot2, idx2, dist, bad);
    }
    static constexpr int kMaxDist = AMOS_TH_LOW - 1;  // :724-726: bestDist1 < TH_LOW, strictly; the same ratio test
};

// ---- SearchForTriangulation
struct TriangulationPolicy {
    struct Query {
        float a, b, c;  // the epipolar line of keyframe 1's feature in keyframe 2 (CheckDistEpipolarLine, :191-193)
        float ex, ey;
        bool stereo;
    };
    static constexpr bool kMatchBySide2 = false;  // match12[idx1] = idx2
    __device__ static bool stereo(const ListSearchArgs &a, int slot, int idx) { return a.uRight && a.uRight[(size_t)slot * a.capacity + idx] >= 0; }
    __device__ static bool query_ok(const ListSearchArgs &a, int slot1, int idx1)
    {
        if (a.hasPoint && a.hasPoint[(size_t)slot1 * a.capacity + idx1]) return false;  // :856-858
        return !a.onlyStereo || stereo(a, slot1, idx1);                                  // :860-864
    }
    __device__ static Query query(const ListSearchArgs &a, int pair, const BowSide &k1, int slot1, int idx1)
    {
        const amos_kf_geometry g = a.geometry[pair];
        const float x = k1.kps[idx1].x, y = k1.kps[idx1].y;
        Query q;
        q.a = __fadd_rn(__fadd_rn(__fmul_rn(x, g.f12[0]), __fmul_rn(y, g.f12[3])), g.f12[6]);
        q.b = __fadd_rn(__fadd_rn(__fmul_rn(x, g.f12[1]), __fmul_rn(y, g.f12[4])), g.f12[7]);
        q.c = __fadd_rn(__fadd_rn(__fmul_rn(x, g.f12[2]), __fmul_rn(y, g.f12[5])), g.f12[8]);
        q.ex = g.ex; q.ey = g.ey;
        q.stereo = stereo(a, slot1, idx1);
        return q;
    }
    // :875-915 without the vbMatched2 test and the running bound: no map point, stereo under onlyStereo, dist <= TH_LOW, then the geometry
    __device__ static bool candidate(const ListSearchArgs &a, const Query &q, const Desc &d1, const BowSide &k2, int slot2, int idx2, int &dist, int &bad)
    {
        if (a.hasPoint && a.hasPoint[(size_t)slot2 * a.capacity + idx2]) return false;
        const bool stereo2 = stereo(a, slot2, idx2);
        if (a.onlyStereo && !stereo2) return false;
        dist = hamming256(d1, load_desc(k2.desc + (size_t)idx2 * 32));
        if (dist > AMOS_TH_LOW) return false;
        const amos_keypoint kp2 = k2.kps[idx2];
        if ((unsigned)kp2.octave >= (unsigned)a.nLevels) { bad = 1; return false; }
        if (!q.stereo && !stereo2) {  // :899-905
            const float distex = __fsub_rn(q.ex, kp2.x), distey = __fsub_rn(q.ey, kp2.y);
            if (__fadd_rn(__fmul_rn(distex, distex), __fmul_rn(distey, distey)) < __fmul_rn(100.0f, a.scale[kp2.octave])) return false;
        }
        const float num = __fadd_rn(__fadd_rn(__fmul_rn(q.a, kp2.x), __fmul_rn(q.b, kp2.y)), q.c);  // :195-208
        const float den = __fadd_rn(__fmul_rn(q.a, q.a), __fmul_rn(q.b, q.b));
        if (den == 0) return false;
        const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
        return (double)dsqr < __dmul_rn(3.84, (double)a.sigma2[kp2.octave]);
    }
    // the LAST of equal distances (dist > bestDist skips, an equal distance replaces)
    __device__ static unsigned key(int dist, int pos) { return ((unsigned)dist << 16) | (unsigned)(0xffff - pos); }
    __device__ static int pos(unsigned key) { return 0xffff - (int)(key & 0xffffu); }
    // only the best is the result: a taken best leaves the second (the best of everything else), and only two taken ask for a new search
    __device__ static Taken taken(const TakenBitmap &t, int bi, int si)
    {
        if (!t.test(bi)) return kKeep;
        if (si < 0) return kNone;
        return t.test(si) ? kAgain : kSecond;
    }
    // no bound (a candidate is within TH_LOW already) and no ratio test: the distances of a record are not even read
    static constexpr int kMaxDist = INT_MAX;
    __device__ static bool ratio_ok(const ListSearchArgs &, int, int) { return true; }
};

// keys -> the record; `it` is the node's list in side 2
template <class P>
__device__ __forceinline__ amos_best2 list_record(unsigned best, unsigned second, const int *it)
{
    amos_best2 r;
    r.best_idx = best == 0xffffffffu ? -1 : it[P::pos(best)];
    r.best_dist = best == 0xffffffffu ? kInitDist : (int)(best >> 16);
    r.second_idx = second == 0xffffffffu ? -1 : it[P::pos(second)];
    r.second_dist = second == 0xffffffffu ? kInitDist : (int)(second >> 16);
    return r;
}

// ---- the candidate loop against side 2 with nothing matched yet.  grid = (ceil(capacity * 8 / 256), pairs), block = 256.
template <class P>
__global__ __launch_bounds__(256) void k_list_best2(const ListSearchArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    const int i1 = t / kWindowLanes, sub = t % kWindowLanes;
    const int slot1 = a.pairs1[p], slot2 = a.pairs2[p];
    const BowSide s1 = bow_side(a, slot1), s2 = bow_side(a, slot2);
    const bool active = i1 < bow_off(a, s1, s1.nNodes);
    int part = -1, b0 = 0, b1 = 0;
    Desc q = {};
    typename P::Query pq = {};
    if (active) {
        int lo = 0, hi = s1.nNodes - 1;  // the last node whose list starts at or before i1
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (bow_off(a, s1, mid) <= i1) lo = mid; else hi = mid - 1;
        }
        const uint32_t id = s1.ids[lo];
        int b = 0, e = s2.nNodes;  // the first node of side 2 with an id >= id
        while (b < e) {
            const int mid = (b + e) >> 1;
            if (s2.ids[mid] < id) b = mid + 1; else e = mid;
        }
        const int idx1 = s1.idx[i1];
        if ((unsigned)idx1 >= (unsigned)s1.n) part = -2;
        else if (b < s2.nNodes && s2.ids[b] == id && P::query_ok(a, slot1, idx1)) {
            part = b;
            b0 = bow_off(a, s2, b);
            b1 = max(bow_off(a, s2, b + 1), b0);
            q = load_desc(s1.desc + (size_t)idx1 * 32);
            pq = P::query(a, p, s1, slot1, idx1);
        }
    }
    unsigned best = 0xffffffffu, second = 0xffffffffu;
    int bad = 0;
    for (int j = b0 + sub; j < b1; j += kWindowLanes) {
        const int idx2 = s2.idx[j];
        if ((unsigned)idx2 >= (unsigned)s2.n) continue;
        int d = 0;
        if (P::candidate(a, pq, q, s2, slot2, idx2, d, bad)) top2_push(best, second, P::key(d, j - b0));
    }
#pragma unroll
    for (int off = kWindowLanes / 2; off > 0; off >>= 1) {
        const unsigned ob = __shfl_xor(best, off, kWindowLanes), os = __shfl_xor(second, off, kWindowLanes);
        top2_merge(best, second, ob, os);
        bad |= __shfl_xor(bad, off, kWindowLanes);
    }
    if (active && sub == 0) {
        const size_t o = (size_t)p * a.capacity + i1;
        a.best2[o] = list_record<P>(best, second, s2.idx + b0);
        a.part[o] = part >= 0 && bad ? part | kPartBadOctave : part;
    }
}

// ---- the sequential loop and the pruning.  One wave per pair walks side 1's list in order with a bitmap of the matched side-2 features
// in LDS.  P::taken says what a prepass record is worth by now; where it asks for it, the whole wave searches the node's list again
// against the bitmap.  Every accepted match is one histogram entry (its bin is kept per query in a.accepted); after the loop every entry
// of a losing bin sets the entry of `match` that its query wrote to -1 and lowers the count.
// Everything the branches read is wave-uniform (read from one lane, or from LDS behind a barrier), so the barriers are reached by all lanes.
template <class P>
__global__ __launch_bounds__(64) void k_list_accept(const ListSearchArgs a)
{
    __shared__ TakenBitmap taken;
    __shared__ int hist[AMOS_HISTO_LENGTH];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int cap = a.capacity;
    const int slot1 = a.pairs1[p], slot2 = a.pairs2[p];
    const BowSide s1 = bow_side(a, slot1), s2 = bow_side(a, slot2);
    const int m1 = bow_off(a, s1, s1.nNodes);
    const bool checkOri = a.checkOri != 0;
    int *match = a.match + (size_t)p * cap;
    const size_t so = (size_t)p * cap;
    for (int w = lane; w < kTakenWords; w += 64) taken.w[w] = 0;
    if (lane < AMOS_HISTO_LENGTH) hist[lane] = 0;
    for (int i = lane; i < cap; i += 64) match[i] = -1;
    __syncthreads();
    int nQueries = 0, nMatches = 0, nResearched = 0, bad = 0;
    for (int base = 0; base < m1; base += 64) {
        const int i1 = base + lane;
        const bool valid = i1 < m1;
        const int part = valid ? a.part[so + i1] : -1;
        bad |= (part == -2 ? 1 : 0) | (part >= 0 && (part & kPartBadOctave) ? 2 : 0);
        amos_best2 rec = list_record<P>(0xffffffffu, 0xffffffffu, nullptr);  // none
        int realIdx = 0;  // this lane's side-1 feature and its angle: read here, side by side, not one by one inside the sequential loop
        float angle = 0.f;
        if (part >= 0) {
            rec = a.best2[so + i1];
            realIdx = s1.idx[i1];  // inside side 1: k_list_best2
            angle = s1.kps[realIdx].angle;
        }
        int acc = -1;  // this lane's query: its entry of a.accepted once it is accepted
        unsigned long long todo = __ballot(part >= 0);
        nQueries += __popcll(todo);
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1;
            int bi = __builtin_amdgcn_readlane(rec.best_idx, k), bd = __builtin_amdgcn_readlane(rec.best_dist, k);
            const int si = __builtin_amdgcn_readlane(rec.second_idx, k);
            int sd = __builtin_amdgcn_readlane(rec.second_dist, k);
            if (bi < 0) continue;  // no candidate in the whole list: none now
            const int idx1 = __builtin_amdgcn_readlane(realIdx, k);
            const Taken tk = P::taken(taken, bi, si);
            if (tk == kNone) continue;
            if (tk == kSecond) { bi = si; bd = sd; }
            if (tk == kAgain) {
                nResearched++;
                const int b = __builtin_amdgcn_readlane(part, k) & kPartNodeMask;
                const int b0 = bow_off(a, s2, b), b1 = max(bow_off(a, s2, b + 1), b0);
                const Desc q = load_desc(s1.desc + (size_t)idx1 * 32);
                const typename P::Query pq = P::query(a, p, s1, slot1, idx1);
                unsigned best, second;
                wave_list_keys(b0, b1, lane, [&](int j) {
                    const int idx2 = s2.idx[j];
                    if ((unsigned)idx2 >= (unsigned)s2.n || taken.test(idx2)) return 0xffffffffu;
                    int d = 0, ignored = 0;
                    return P::candidate(a, pq, q, s2, slot2, idx2, d, ignored) ? P::key(d, j - b0) : 0xffffffffu;
                }, best, second);
                const amos_best2 r = list_record<P>(best, second, s2.idx + b0);
                if (r.best_idx < 0) continue;
                bi = r.best_idx; bd = r.best_dist; sd = r.second_dist;
            }
            if (bd > P::kMaxDist) continue;  // (on its own: a scalar comparison ends most queries)
            if (!P::ratio_ok(a, bd, sd)) continue;
            nMatches++;
            int bin = 0;
            if (checkOri) bin = rotation_bin(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(angle), k)), s2.kps[bi].angle);
            if (lane == k) acc = P::kMatchBySide2 ? (bin << 16) | bi : bin;
            if (lane == 0) {
                match[P::kMatchBySide2 ? bi : idx1] = P::kMatchBySide2 ? idx1 : bi;  // (either entry is written once)
                taken.set(bi);
                if (checkOri) hist[bin]++;
            }
            __syncthreads();  // the bit is visible to every lane before the next query reads the bitmap
        }
        if (valid) a.accepted[so + i1] = acc;
    }
    __threadfence_block();
    __syncthreads();  // lane 0's writes to match and hist are over before the pruning reads and overwrites
    if (checkOri) {
        int ind1, ind2, ind3;
        three_maxima(hist, ind1, ind2, ind3);
        int pruned = 0;
        for (int base = 0; base < m1; base += 64) {
            const int i1 = base + lane;
            const int acc = i1 < m1 ? a.accepted[so + i1] : -1;
            const int bin = P::kMatchBySide2 ? acc >> 16 : acc;
            const bool lose = acc >= 0 && bin != ind1 && bin != ind2 && bin != ind3;
            if (lose) match[P::kMatchBySide2 ? acc & 0xffff : s1.idx[i1]] = -1;  // (an accepted query's feature index lies inside side 1)
            pruned += __popcll(__ballot(lose));
        }
        nMatches -= pruned;
    }
    const unsigned long long bad0 = __ballot(bad & 1), bad1 = __ballot(bad & 2);
    if (lane == 0) {
        amos_bow_search_stats s;
        s.n_queries = nQueries; s.n_matches = nMatches; s.n_researched = nResearched; s.status = (bad0 ? 1 : 0) | (bad1 ? 2 : 0);
        a.stats[p] = s;
    }
}

// what the two public structs name differently
static void fill_pair_args(ListSearchArgs &a, const amos_bow_search &s) { a.pairs1 = s.d_pairs_kf; a.pairs2 = s.d_pairs_f; a.match = s.d_match; a.uRight = nullptr; }
static void fill_pair_args(ListSearchArgs &a, const amos_kf_pair_search &s) { a.pairs1 = s.d_pairs_1; a.pairs2 = s.d_pairs_2; a.match = s.d_match12; a.uRight = s.d_u_right; }

// S: amos_bow_search or amos_kf_pair_search
template <class S>
static void fill_list_args(ListSearchArgs &a, const S &s)
{
    a.kps = s.d_kps; a.desc = s.d_desc; a.counts = s.d_counts; a.nNodes = s.d_n_nodes; a.nodeIds = s.d_node_ids; a.nodeOff = s.d_node_off;
    a.nodeIdx = s.d_node_idx; a.hasPoint = s.d_has_point; a.stats = s.d_stats; a.capacity = s.capacity;
    fill_pair_args(a, s);
}

// The check every batch entry makes (own: the entry's own arguments are there), the scratch of a call and the two launches; `a` comes with
// the entry's own parameters.
template <class P, class S>
static int launch_pair_search(const char *name, amos_match *m, const S *s, bool own, ListSearchArgs &a)
{
    if (m && s) fill_list_args(a, *s);
    if (!m || !s || !own || !a.kps || !a.desc || !a.counts || !a.nNodes || !a.nodeIds || !a.nodeOff || !a.nodeIdx || !a.pairs1 || !a.pairs2 ||
        !a.match || !a.stats || s->n_pairs < 1 || s->capacity < 1 || s->capacity > 65536) {
        set_error("%s: invalid argument", name);
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t total = (size_t)s->n_pairs * s->capacity;
    const size_t bytesBest = align64(sizeof(amos_best2) * total), bytesInt = align64(sizeof(int) * total);
    int rc = grow(&m->dLocal, &m->capLocal, bytesBest + 2 * bytesInt);
    if (rc != AMOS_OK) return rc;
    a.best2 = (amos_best2 *)m->dLocal; a.part = (int *)(m->dLocal + bytesBest); a.accepted = (int *)(m->dLocal + bytesBest + bytesInt);
    hipLaunchKernelGGL(k_list_best2<P>, dim3(((size_t)s->capacity * kWindowLanes + 255) / 256, s->n_pairs), dim3(256), 0, m->stream, a);
    hipLaunchKernelGGL(k_list_accept<P>, dim3(s->n_pairs), dim3(64), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

// ---- the host forms: nv views as frame slots of one capacity, nPairs pairs of them, one upload, one batch call, one download

static size_t staged_view_bytes(int nv, size_t cap) { return (size_t)nv * (cap * (sizeof(amos_keypoint) + 32 + 4 + 4 + 4 + 1 + 4) + 4 + 64 * 10) + 1024; }
static size_t pair_match_bytes(size_t cap, int nPairs) { return align64(sizeof(int32_t) * cap * nPairs); }
static size_t pair_out_bytes(size_t cap, int nPairs) { return pair_match_bytes(cap, nPairs) + align64(sizeof(amos_bow_search_stats) * nPairs); }

// The staging arena for the views, `ownBytes` of the form's own inputs and the download; dOut for match [nPairs][cap] and stats [nPairs],
// and `extraOut` bytes of the form's own results behind them.
static int host_pairs_begin(amos_match *m, int nv, size_t cap, int nPairs, size_t ownBytes, size_t extraOut = 0)
{
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    int rc = stage_begin(m, staged_view_bytes(nv, cap) + ownBytes + pair_out_bytes(cap, nPairs) + extraOut);
    if (rc != AMOS_OK) return rc;
    return grow_out(m, pair_out_bytes(cap, nPairs) + extraOut);
}

// The views staged for ONE upload: a view's arrays at the front of its slot, zeros behind; has_point and u_right are staged when any
// view has them (a view without gets `hpNone` / -1).  Fills s but for its pairs; the pairs' results lie in dOut.
static void stage_views(amos_match *m, const amos_bow_view *const *views, int nv, size_t cap, int nPairs, uint8_t hpNone, bool wantRight,
                        amos_kf_pair_search &s)
{
    auto all = [&](size_t per, size_t elem, auto src, auto count) {
        const size_t o = stage_take(m, nv * per * elem);
        std::memset(m->hStage + o, 0, nv * per * elem);
        for (int v = 0; v < nv; v++) {
            const void *p = src(*views[v]);
            const size_t c = count(*views[v]);
            if (p && c) std::memcpy(m->hStage + o + v * per * elem, p, c * elem);
        }
        return o;
    };
    auto nFeat = [](const amos_bow_view &v) { return (size_t)v.n; };
    auto nNode = [](const amos_bow_view &v) { return (size_t)v.n_nodes; };
    s.d_kps = (const amos_keypoint *)(m->dArena + all(cap, sizeof(amos_keypoint), [](const amos_bow_view &v) { return (const void *)v.keys; }, nFeat));
    s.d_desc = m->dArena + all(cap, 32, [](const amos_bow_view &v) { return (const void *)v.descriptors; }, nFeat);
    s.d_node_ids = (const uint32_t *)(m->dArena + all(cap, 4, [](const amos_bow_view &v) { return (const void *)v.node_ids; }, nNode));
    s.d_node_off = (const int32_t *)(m->dArena + all(cap + 1, 4, [](const amos_bow_view &v) { return (const void *)v.node_off; },
                                                     [](const amos_bow_view &v) { return v.n_nodes ? (size_t)v.n_nodes + 1 : 0; }));
    s.d_node_idx = (const int32_t *)(m->dArena + all(cap, 4, [](const amos_bow_view &v) { return (const void *)v.node_idx; },
                                                     [](const amos_bow_view &v) { return v.n_nodes ? (size_t)v.node_off[v.n_nodes] : 0; }));
    bool anyPoint = false, anyRight = false;
    for (int v = 0; v < nv; v++) { anyPoint |= views[v]->has_point != nullptr; anyRight |= views[v]->u_right != nullptr; }
    s.d_has_point = nullptr;
    if (anyPoint) {
        const size_t o = all(cap, 1, [](const amos_bow_view &v) { return (const void *)v.has_point; }, nFeat);
        for (int v = 0; v < nv; v++) if (!views[v]->has_point) std::memset(m->hStage + o + v * cap, hpNone, cap);
        s.d_has_point = m->dArena + o;
    }
    s.d_u_right = nullptr;
    if (wantRight && anyRight) {
        const size_t o = all(cap, 4, [](const amos_bow_view &v) { return (const void *)v.u_right; }, nFeat);
        float *h = (float *)(m->hStage + o);
        for (int v = 0; v < nv; v++) if (!views[v]->u_right) std::fill(h + v * cap, h + (v + 1) * cap, -1.0f);
        s.d_u_right = (const float *)(m->dArena + o);
    }
    std::vector<int32_t> counts(nv), nodes(nv);
    for (int v = 0; v < nv; v++) { counts[v] = views[v]->n; nodes[v] = views[v]->n_nodes; }
    s.d_counts = stage_input<int32_t>(m, counts.data(), sizeof(int32_t) * nv);
    s.d_n_nodes = stage_input<int32_t>(m, nodes.data(), sizeof(int32_t) * nv);
    s.d_match12 = (int32_t *)m->dOut;
    s.d_stats = (amos_bow_search_stats *)((uint8_t *)m->dOut + pair_match_bytes(cap, nPairs));
    s.n_pairs = nPairs; s.capacity = (int32_t)cap;
}

// One download of the pairs' results through the staging buffer: the first n entries of every pair's row of `match`, and the stats.
static int download_pairs(amos_match *m, size_t cap, int nPairs, int n, int32_t *match, amos_bow_search_stats *stats)
{
    const size_t bytes = pair_out_bytes(cap, nPairs);
    const uint8_t *h = m->hStage + stage_take(m, bytes);
    AMOS_HIP_CHECK(hipMemcpyAsync((void *)h, m->dOut, bytes, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    for (int v = 0; v < nPairs && n; v++) std::memcpy(match + (size_t)v * n, h + sizeof(int32_t) * cap * v, sizeof(int32_t) * (size_t)n);
    std::memcpy(stats, h + pair_match_bytes(cap, nPairs), sizeof(amos_bow_search_stats) * nPairs);
    return AMOS_OK;
}

// The two-view forms: slot 0 against slot 1; n entries of the result go to `match`.
template <class P>
static int host_two_views(const char *name, amos_match *m, const amos_bow_view *v1, const amos_bow_view *v2, float nn_ratio, int check_orientation,
                          int n, int32_t *match, amos_bow_search_stats *stats)
{
    if (!m || !stats || !bow_view_ok(v1) || !bow_view_ok(v2) || (n > 0 && !match)) {
        set_error("%s: invalid argument (a NULL pointer, or a view whose node ids, offsets or feature indices are out of order or range)", name);
        return AMOS_ERR_INVALID;
    }
    const size_t cap = (size_t)std::max(std::max(v1->n, v2->n), 1);
    int rc = host_pairs_begin(m, 2, cap, 1, 0);
    if (rc != AMOS_OK) return rc;
    const amos_bow_view *views[2] = {v1, v2};
    amos_kf_pair_search s;
    stage_views(m, views, 2, cap, 1, 1, false, s);
    const int32_t slots[2] = {0, 1};
    s.d_pairs_1 = stage_input<int32_t>(m, slots, sizeof(slots));
    s.d_pairs_2 = s.d_pairs_1 + 1;
    ListSearchArgs a = {};
    a.nnRatio = nn_ratio; a.checkOri = check_orientation;
    if ((rc = stage_flush(m)) != AMOS_OK || (rc = launch_pair_search<P>(name, m, &s, true, a)) != AMOS_OK) return rc;
    return download_pairs(m, cap, 1, n, match, stats);
}

}  // namespace amos

using namespace amos;

extern "C" {

int amos_match_bow_batch_device(amos_match *m, const amos_bow_search *s)
{
    ListSearchArgs a = {};
    if (s) { a.nnRatio = s->nn_ratio; a.checkOri = s->check_orientation; }
    return launch_pair_search<BowFramePolicy>("amos_match_bow_batch_device", m, s, true, a);
}

int amos_match_bow_kf_batch_device(amos_match *m, const amos_kf_pair_search *s, float nn_ratio, int check_orientation)
{
    ListSearchArgs a = {};
    a.nnRatio = nn_ratio; a.checkOri = check_orientation;
    return launch_pair_search<BowKfPolicy>("amos_match_bow_kf_batch_device", m, s, true, a);
}

int amos_match_triangulation_batch_device(amos_match *m, const amos_kf_pair_search *s, const amos_kf_geometry *d_geometry,
                                          const float *d_scale_factors, const float *d_level_sigma2, int n_levels, int only_stereo,
                                          int check_orientation)
{
    ListSearchArgs a = {};
    a.geometry = d_geometry; a.scale = d_scale_factors; a.sigma2 = d_level_sigma2; a.nLevels = n_levels;
    a.onlyStereo = only_stereo; a.checkOri = check_orientation;
    const bool own = d_geometry && d_scale_factors && d_level_sigma2 && n_levels >= 1 && n_levels <= AMOS_MAX_LEVELS;
    return launch_pair_search<TriangulationPolicy>("amos_match_triangulation_batch_device", m, s, own, a);
}

int amos_match_bow(amos_match *m, const amos_bow_view *kf, const amos_bow_view *f, float nn_ratio, int check_orientation, int32_t *matches_f,
                   amos_bow_search_stats *stats)
{
    return host_two_views<BowFramePolicy>("amos_match_bow", m, kf, f, nn_ratio, check_orientation, f ? f->n : 0, matches_f, stats);
}

int amos_match_bow_kf(amos_match *m, const amos_bow_view *k1, const amos_bow_view *k2, float nn_ratio, int check_orientation, int32_t *match12,
                      amos_bow_search_stats *stats)
{
    return host_two_views<BowKfPolicy>("amos_match_bow_kf", m, k1, k2, nn_ratio, check_orientation, k1 ? k1->n : 0, match12, stats);
}

int amos_match_triangulation(amos_match *m, const amos_bow_view *k1, const amos_bow_view *const *k2s, int n2, const amos_kf_geometry *geometry,
                             const float *scale_factors, const float *level_sigma2, int n_levels, int only_stereo, int check_orientation,
                             int32_t *match12, amos_bow_search_stats *stats)
{
    bool ok = m && stats && k2s && n2 >= 1 && geometry && scale_factors && level_sigma2 && n_levels >= 1 && n_levels <= AMOS_MAX_LEVELS &&
              bow_view_ok(k1) && (k1->n == 0 || match12);
    for (int v = 0; ok && v < n2; v++) ok = bow_view_ok(k2s[v]);
    if (!ok) {
        set_error("amos_match_triangulation: invalid argument (a NULL pointer, n2 or n_levels out of range, or a view whose node ids, offsets or "
                  "feature indices are out of order or range)");
        return AMOS_ERR_INVALID;
    }
    size_t cap = (size_t)std::max(k1->n, 1);
    for (int v = 0; v < n2; v++) cap = std::max(cap, (size_t)k2s[v]->n);
    const int nv = n2 + 1;
    int rc = host_pairs_begin(m, nv, cap, n2, (size_t)n2 * (sizeof(amos_kf_geometry) + 8) + 2 * 64 * (AMOS_MAX_LEVELS / 16 + 1) + 256);
    if (rc != AMOS_OK) return rc;
    std::vector<const amos_bow_view *> views(nv);
    views[0] = k1;  // keyframe 1 is slot 0, staged once for all pairs
    for (int v = 0; v < n2; v++) views[v + 1] = k2s[v];
    amos_kf_pair_search s;
    stage_views(m, views.data(), nv, cap, n2, 0, true, s);
    std::vector<int32_t> slots(2 * (size_t)n2, 0);
    for (int v = 0; v < n2; v++) slots[n2 + v] = v + 1;
    s.d_pairs_1 = stage_input<int32_t>(m, slots.data(), sizeof(int32_t) * 2 * n2);
    s.d_pairs_2 = s.d_pairs_1 + n2;
    const amos_kf_geometry *dGeo = stage_input<amos_kf_geometry>(m, geometry, sizeof(amos_kf_geometry) * n2);
    const float *dScale = stage_input<float>(m, scale_factors, sizeof(float) * n_levels);
    const float *dSigma = stage_input<float>(m, level_sigma2, sizeof(float) * n_levels);
    if ((rc = stage_flush(m)) != AMOS_OK ||
        (rc = amos_match_triangulation_batch_device(m, &s, dGeo, dScale, dSigma, n_levels, only_stereo, check_orientation)) != AMOS_OK) return rc;
    return download_pairs(m, cap, n2, k1->n, match12, stats);
}

// CreateNewMapPoints up to its `new MapPoint` for one keyframe 1 and n2 neighbours: geometry and baseline gate per neighbour on the host,
// the kept neighbours staged like amos_match_triangulation's, the search's two launches and amos_match_new_points_batch_device's two on
// the stream, one download of the new-point records and their stats.
int amos_match_new_points(amos_match *m, const amos_bow_view *k1, const amos_bow_view *const *k2s, int n2, const amos_kf_camera *cam1,
                          const amos_kf_camera *cams2, const amos_keypoint *kps_raw1, const amos_keypoint *const *kps_raw2, const float *depth1,
                          const float *const *depth2, const float *scale_factors, const float *level_sigma2, int n_levels, int only_stereo,
                          int check_orientation, amos_new_point *new_points, amos_new_points_stats *stats)
{
    bool ok = m && stats && k2s && n2 >= 1 && n2 <= AMOS_NEW_POINTS_MAX_PAIRS && cam1 && cams2 && scale_factors && level_sigma2 && n_levels >= 1 &&
              n_levels <= AMOS_MAX_LEVELS && bow_view_ok(k1) && (k1->n == 0 || new_points) && (k1->n == 0 || !k1->u_right || depth1);
    for (int v = 0; ok && v < n2; v++) ok = bow_view_ok(k2s[v]) && (k2s[v]->n == 0 || !k2s[v]->u_right || (depth2 && depth2[v]));
    if (!ok) {
        set_error("amos_match_new_points: invalid argument (a NULL pointer, n2 or n_levels out of range, a stereo view without depths, or a view "
                  "whose node ids, offsets or feature indices are out of order or range)");
        return AMOS_ERR_INVALID;
    }
    std::vector<int> kept;
    std::vector<amos_kf_geometry> geo;
    std::vector<amos_kf_camera> cams(1, *cam1);
    for (int v = 0; v < n2; v++) {
        amos_kf_geometry g;
        if (amos_kf_geometry_from_poses(cam1, cams2 + v, &g) != 1) continue;  // the baseline gate
        kept.push_back(v);
        geo.push_back(g);
        cams.push_back(cams2[v]);
    }
    std::memset(stats, 0, sizeof(amos_new_points_stats) * (size_t)n2);
    const int nk = (int)kept.size(), nv = nk + 1;
    if (nk == 0) return AMOS_OK;
    size_t cap = (size_t)std::max(k1->n, 1);
    for (int v : kept) cap = std::max(cap, (size_t)k2s[v]->n);
    const size_t bytesNew = align64(sizeof(amos_new_point) * cap * nk), bytesStats = align64(sizeof(amos_new_points_stats) * (size_t)nk);
    int rc = host_pairs_begin(m, nv, cap, nk,
                              (size_t)nk * (sizeof(amos_kf_geometry) + 8) + 2 * 64 * (AMOS_MAX_LEVELS / 16 + 1) + 256 +
                                  (size_t)nv * (cap * (sizeof(amos_keypoint) + 4) + 128) + bytesNew + bytesStats,
                              bytesNew + bytesStats);
    if (rc != AMOS_OK) return rc;
    std::vector<const amos_bow_view *> views(nv);
    std::vector<const amos_keypoint *> raws(nv);
    std::vector<const float *> depths(nv);
    views[0] = k1; raws[0] = kps_raw1; depths[0] = depth1;
    bool anyRaw = kps_raw1 != nullptr;
    for (int i = 0; i < nk; i++) {
        views[i + 1] = k2s[kept[i]];
        raws[i + 1] = kps_raw2 ? kps_raw2[kept[i]] : nullptr;
        depths[i + 1] = depth2 ? depth2[kept[i]] : nullptr;
        anyRaw |= raws[i + 1] != nullptr;
    }
    amos_kf_pair_search s;
    stage_views(m, views.data(), nv, cap, nk, 0, true, s);
    std::vector<int32_t> slots(2 * (size_t)nk, 0);
    for (int i = 0; i < nk; i++) slots[nk + i] = i + 1;
    s.d_pairs_1 = stage_input<int32_t>(m, slots.data(), sizeof(int32_t) * 2 * nk);
    s.d_pairs_2 = s.d_pairs_1 + nk;
    const amos_kf_geometry *dGeo = stage_input<amos_kf_geometry>(m, geo.data(), sizeof(amos_kf_geometry) * nk);
    const float *dScale = stage_input<float>(m, scale_factors, sizeof(float) * n_levels);
    const float *dSigma = stage_input<float>(m, level_sigma2, sizeof(float) * n_levels);
    amos_new_points q = {};
    if (anyRaw) {  // a view without raw keypoints of its own: its keys
        const size_t o = stage_take(m, nv * cap * sizeof(amos_keypoint));
        std::memset(m->hStage + o, 0, nv * cap * sizeof(amos_keypoint));
        for (int v = 0; v < nv; v++)
            if (views[v]->n) std::memcpy(m->hStage + o + v * cap * sizeof(amos_keypoint), raws[v] ? raws[v] : views[v]->keys, sizeof(amos_keypoint) * (size_t)views[v]->n);
        q.d_kps_raw = (const amos_keypoint *)(m->dArena + o);
    }
    if (s.d_u_right) {
        const size_t o = stage_take(m, nv * cap * sizeof(float));
        float *h = (float *)(m->hStage + o);
        std::fill(h, h + nv * cap, -1.0f);
        for (int v = 0; v < nv; v++)
            if (views[v]->n && depths[v]) std::memcpy(h + v * cap, depths[v], sizeof(float) * (size_t)views[v]->n);
        q.d_depth = (const float *)(m->dArena + o);
    }
    uint8_t *out = (uint8_t *)m->dOut + pair_out_bytes(cap, nk);
    q.d_kps = s.d_kps; q.d_counts = s.d_counts; q.d_u_right = s.d_u_right; q.d_pairs_1 = s.d_pairs_1; q.d_pairs_2 = s.d_pairs_2;
    q.d_match12 = s.d_match12; q.d_scale_factors = dScale; q.d_level_sigma2 = dSigma; q.cameras = cams.data();
    q.pairs_1 = slots.data(); q.pairs_2 = slots.data() + nk; q.enabled = nullptr;
    q.d_new = (amos_new_point *)out; q.d_verdict = nullptr; q.d_stats = (amos_new_points_stats *)(out + bytesNew);
    q.n_frames = nv; q.n_pairs = nk; q.capacity = (int32_t)cap; q.n_levels = n_levels;
    if ((rc = stage_flush(m)) != AMOS_OK ||
        (rc = amos_match_triangulation_batch_device(m, &s, dGeo, dScale, dSigma, n_levels, only_stereo, check_orientation)) != AMOS_OK ||
        (rc = amos_match_new_points_batch_device(m, &q)) != AMOS_OK) return rc;
    const uint8_t *h = m->hStage + stage_take(m, bytesNew + bytesStats);
    AMOS_HIP_CHECK(hipMemcpyAsync((void *)h, out, bytesNew + bytesStats, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    const amos_new_points_stats *st = (const amos_new_points_stats *)(h + bytesNew);
    for (int i = 0; i < nk; i++) {
        stats[kept[i]] = st[i];
        const size_t n = (size_t)std::min(std::max(st[i].n_new, 0), k1->n);
        if (n) std::memcpy(new_points + (size_t)kept[i] * k1->n, h + sizeof(amos_new_point) * cap * i, sizeof(amos_new_point) * n);
    }
    return AMOS_OK;
}

}  // extern "C"
