// amos_bow_search.hip -- ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vpMapPointMatches) (ORBmatcher.cc:230-382) for a batch of
// (keyframe, frame) pairs of resident frames whose FeatureVectors are the CSR of amos_bow_transform_batch_device (amos_bow.hip).
//
// Launches on the matcher's stream: k_bow_best2 (eight lanes per keyframe feature: the best two frame features of its node, taken or not)
// and k_bow_accept (one wave per pair: the reference's sequential loop over those records, then the rotation histogram's pruning).  The
// semantics are defined in include/amos_frontend.h, "bag of words".
#include "amos_bow_list.h"  // BowSide, the wave's list search, bow_view_ok

#include <vector>

namespace amos {

static_assert(sizeof(amos_bow_search_stats) == 16, "amos_bow_search_stats is 16 bytes (include/amos_frontend.h)");

struct BowSearchArgs {
    const amos_keypoint *kps;
    const uint8_t *desc;
    const int *counts, *nNodes;
    const uint32_t *nodeIds;
    const int *nodeOff, *nodeIdx;
    const uint8_t *hasPoint;
    const int *pairsKf, *pairsF;
    int *match;
    amos_bow_search_stats *stats;
    amos_best2 *best2;  // scratch, per pair and keyframe list position: the prepass record (indices are frame features)
    int *part;          // scratch, alike: the frame's node (its place in the frame's node list) the query searches, -1: none (its node is
                        // not shared, or no map point), -2: a feature index outside the keyframe
    int *accepted;      // scratch, alike: -1, or bin << 16 | frame feature of the query's accepted match
    int capacity;
    float nnRatio;
    int checkOri;
};

// ---- the candidate loop of ORBmatcher.cc:278-304 against the frame with nothing matched yet (list order is candidate order: the first of
// equal distances wins).  grid = (ceil(capacity * 8 / 256), pairs), block = 256.
__global__ __launch_bounds__(256) void k_bow_best2(const BowSearchArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    const int ik = t / kWindowLanes, sub = t % kWindowLanes;
    const int slotKf = a.pairsKf[p];
    const BowSide kf = bow_side(a, slotKf), fr = bow_side(a, a.pairsF[p]);
    const bool active = ik < bow_off(a, kf, kf.nNodes);
    int part = -1, b0 = 0, b1 = 0;
    Desc q = {};
    if (active) {
        int lo = 0, hi = kf.nNodes - 1;  // the last node whose list starts at or before ik
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (bow_off(a, kf, mid) <= ik) lo = mid; else hi = mid - 1;
        }
        const uint32_t id = kf.ids[lo];
        int b = 0, e = fr.nNodes;  // the first frame node with an id >= id
        while (b < e) {
            const int mid = (b + e) >> 1;
            if (fr.ids[mid] < id) b = mid + 1; else e = mid;
        }
        const int realIdxKF = kf.idx[ik];
        if ((unsigned)realIdxKF >= (unsigned)kf.n) part = -2;
        else if (b < fr.nNodes && fr.ids[b] == id && (!a.hasPoint || a.hasPoint[(size_t)slotKf * a.capacity + realIdxKF])) {
            part = b;
            b0 = bow_off(a, fr, b);
            b1 = max(bow_off(a, fr, b + 1), b0);
            q = load_desc(kf.desc + (size_t)realIdxKF * 32);
        }
    }
    unsigned best = 0xffffffffu, second = 0xffffffffu;
    for (int j = b0 + sub; j < b1; j += kWindowLanes) {
        const int idx = fr.idx[j];
        if ((unsigned)idx >= (unsigned)fr.n) continue;
        const int d = hamming256(q, load_desc(fr.desc + (size_t)idx * 32));
        if (d < kInitDist) top2_push(best, second, ((unsigned)d << 16) | (unsigned)(j - b0));
    }
#pragma unroll
    for (int off = kWindowLanes / 2; off > 0; off >>= 1) {
        const unsigned ob = __shfl_xor(best, off, kWindowLanes), os = __shfl_xor(second, off, kWindowLanes);
        top2_merge(best, second, ob, os);
    }
    if (active && sub == 0) {
        const size_t o = (size_t)p * a.capacity + ik;
        a.best2[o] = best2_from_keys(best, second, fr.idx + b0, kInitDist);
        a.part[o] = part;
    }
}

// ---- the sequential loop of ORBmatcher.cc:254-345 and the pruning of :348-361.  One wave per pair walks the keyframe's list in order with
// a bitmap of the matched frame features in LDS.  The prepass record stands when neither of its two is matched; otherwise the whole wave
// searches the node's list again against the bitmap.  Every accepted match is one histogram entry (its frame feature and bin are kept per
// query in a.accepted); after the loop every entry of a losing bin sets its frame feature to -1 and lowers the count.
// Everything the branches read is wave-uniform (read from one lane, or from LDS behind a barrier), so the barriers are reached by all lanes.
__global__ __launch_bounds__(64) void k_bow_accept(const BowSearchArgs a)
{
    __shared__ TakenBitmap taken;
    __shared__ int hist[AMOS_HISTO_LENGTH];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int cap = a.capacity;
    const BowSide kf = bow_side(a, a.pairsKf[p]), fr = bow_side(a, a.pairsF[p]);
    const int mKf = bow_off(a, kf, kf.nNodes);
    const bool checkOri = a.checkOri != 0;
    int *match = a.match + (size_t)p * cap;
    const size_t so = (size_t)p * cap;
    for (int w = lane; w < kTakenWords; w += 64) taken.w[w] = 0;
    if (lane < AMOS_HISTO_LENGTH) hist[lane] = 0;
    for (int i = lane; i < cap; i += 64) match[i] = -1;
    __syncthreads();
    const float factor = AMOS_HISTO_LENGTH / 360.0f;
    int nQueries = 0, nMatches = 0, nResearched = 0, bad = 0;
    for (int base = 0; base < mKf; base += 64) {
        const int ik = base + lane;
        const bool valid = ik < mKf;
        const int part = valid ? a.part[so + ik] : -1;
        bad |= part == -2;
        amos_best2 rec = best2_from_keys(0xffffffffu, 0xffffffffu, nullptr, kInitDist);  // none
        int realIdx = 0;    // this lane's keyframe feature and its angle: read here, side by side, not one by one inside the sequential loop
        float angle = 0.f;
        if (part >= 0) {
            rec = a.best2[so + ik];
            realIdx = kf.idx[ik];  // inside the keyframe: k_bow_best2
            angle = kf.kps[realIdx].angle;
        }
        int acc = -1;  // this lane's query: bin << 16 | frame feature once it is accepted
        unsigned long long todo = __ballot(part >= 0);
        nQueries += __popcll(todo);
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1;
            int bi = __builtin_amdgcn_readlane(rec.best_idx, k), bd = __builtin_amdgcn_readlane(rec.best_dist, k);
            const int si = __builtin_amdgcn_readlane(rec.second_idx, k);
            int sd = __builtin_amdgcn_readlane(rec.second_dist, k);
            if (bi < 0) continue;  // no candidate below 256 in the whole list: none now
            const int realIdxKF = __builtin_amdgcn_readlane(realIdx, k);
            if (taken.either(bi, si)) {
                nResearched++;
                const int b = __builtin_amdgcn_readlane(part, k);
                const int b0 = bow_off(a, fr, b), b1 = max(bow_off(a, fr, b + 1), b0);
                const amos_best2 r = wave_list_best2(fr, b0, b1, load_desc(kf.desc + (size_t)realIdxKF * 32), taken, lane);
                if (r.best_idx < 0) continue;
                bi = r.best_idx; bd = r.best_dist; sd = r.second_dist;
            }
            if (bd > AMOS_TH_LOW || !((float)bd < __fmul_rn(a.nnRatio, (float)sd))) continue;  // :306-309
            nMatches++;
            int bin = 0;
            if (checkOri) {  // :314-323
                float rot = __fsub_rn(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(angle), k)), fr.kps[bi].angle);
                if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
                bin = (int)roundf(__fmul_rn(rot, factor));
                if (bin == AMOS_HISTO_LENGTH) bin = 0;
                bin = min(max(bin, 0), AMOS_HISTO_LENGTH - 1);  // (the reference asserts it; an angle that is not finite lands in bin 0)
            }
            if (lane == k) acc = (bin << 16) | bi;
            if (lane == 0) {
                match[bi] = realIdxKF;
                taken.set(bi);
                if (checkOri) hist[bin]++;
            }
            __syncthreads();  // the bit is visible to every lane before the next query reads the bitmap
        }
        if (valid) a.accepted[so + ik] = acc;
    }
    __threadfence_block();
    __syncthreads();  // lane 0's writes to match and hist are over before the pruning reads and overwrites
    if (checkOri) {
        // ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1866-1908): strict comparisons, the earlier bin wins a tie
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < AMOS_HISTO_LENGTH; i++) {
            const int s = hist[i];
            if (s > max1) {
                max3 = max2; max2 = max1; max1 = s;
                ind3 = ind2; ind2 = ind1; ind1 = i;
            } else if (s > max2) {
                max3 = max2; max2 = s;
                ind3 = ind2; ind2 = i;
            } else if (s > max3) {
                max3 = s; ind3 = i;
            }
        }
        if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }
        else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) ind3 = -1;
        int pruned = 0;
        for (int base = 0; base < mKf; base += 64) {
            const int ik = base + lane;
            const int acc = ik < mKf ? a.accepted[so + ik] : -1;
            const int bin = acc >> 16;
            const bool lose = acc >= 0 && bin != ind1 && bin != ind2 && bin != ind3;
            if (lose) match[acc & 0xffff] = -1;
            pruned += __popcll(__ballot(lose));
        }
        nMatches -= pruned;
    }
    const unsigned long long anyBad = __ballot(bad != 0);
    if (lane == 0) {
        amos_bow_search_stats s;
        s.n_queries = nQueries; s.n_matches = nMatches; s.n_researched = nResearched; s.status = anyBad ? 1 : 0;
        a.stats[p] = s;
    }
}

}  // namespace amos

using namespace amos;

extern "C" {

int amos_match_bow_batch_device(amos_match *m, const amos_bow_search *s)
{
    if (!m || !s || !s->d_kps || !s->d_desc || !s->d_counts || !s->d_n_nodes || !s->d_node_ids || !s->d_node_off || !s->d_node_idx ||
        !s->d_pairs_kf || !s->d_pairs_f || !s->d_match || !s->d_stats || s->n_pairs < 1 || s->capacity < 1 || s->capacity > 65536) {
        set_error("amos_match_bow_batch_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t total = (size_t)s->n_pairs * s->capacity;
    const size_t bytesBest = align64(sizeof(amos_best2) * total), bytesInt = align64(sizeof(int) * total);
    int rc = grow(&m->dLocal, &m->capLocal, bytesBest + 2 * bytesInt);
    if (rc != AMOS_OK) return rc;
    BowSearchArgs a;
    a.kps = s->d_kps; a.desc = s->d_desc; a.counts = s->d_counts; a.nNodes = s->d_n_nodes; a.nodeIds = s->d_node_ids; a.nodeOff = s->d_node_off;
    a.nodeIdx = s->d_node_idx; a.hasPoint = s->d_has_point; a.pairsKf = s->d_pairs_kf; a.pairsF = s->d_pairs_f;
    a.match = s->d_match; a.stats = s->d_stats;
    a.best2 = (amos_best2 *)m->dLocal; a.part = (int *)(m->dLocal + bytesBest); a.accepted = (int *)(m->dLocal + bytesBest + bytesInt);
    a.capacity = s->capacity; a.nnRatio = s->nn_ratio; a.checkOri = s->check_orientation;
    hipLaunchKernelGGL(k_bow_best2, dim3(((size_t)s->capacity * kWindowLanes + 255) / 256, s->n_pairs), dim3(256), 0, m->stream, a);
    hipLaunchKernelGGL(k_bow_accept, dim3(s->n_pairs), dim3(64), 0, m->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_match_bow(amos_match *m, const amos_bow_view *kf, const amos_bow_view *f, float nn_ratio, int check_orientation, int32_t *matches_f,
                   amos_bow_search_stats *stats)
{
    if (!m || !stats || !bow_view_ok(kf) || !bow_view_ok(f) || (f->n > 0 && !matches_f)) {
        set_error("amos_match_bow: invalid argument (a NULL pointer, or a view whose node ids, offsets or feature indices are out of order or range)");
        return AMOS_ERR_INVALID;
    }
    AMOS_HIP_CHECK(hipSetDevice(m->device));
    const size_t cap = (size_t)std::max(std::max(kf->n, f->n), 1);
    const size_t bytesMatch = align64(sizeof(int32_t) * cap), bytesOut = bytesMatch + align64(sizeof(amos_bow_search_stats));
    const size_t perSlot = cap * (sizeof(amos_keypoint) + 32 + 4 + 4 + 4 + 1) + 4 + 64 * 8;
    int rc = stage_begin(m, 2 * perSlot + 1024 + bytesOut);
    if (rc != AMOS_OK) return rc;
    rc = grow_out(m, bytesOut);
    if (rc != AMOS_OK) return rc;
    const amos_bow_view *views[2] = {kf, f};
    // an array of both slots, [2][per]: the views' parts at the front of each slot, zeros behind
    auto both = [&](size_t per, size_t elem, auto src, auto count) {
        const size_t o = stage_take(m, 2 * per * elem);
        std::memset(m->hStage + o, 0, 2 * per * elem);
        for (int v = 0; v < 2; v++) {
            const void *p = src(*views[v]);
            const size_t c = count(*views[v]);
            if (p && c) std::memcpy(m->hStage + o + v * per * elem, p, c * elem);
        }
        return m->dArena + o;
    };
    auto nFeat = [](const amos_bow_view &v) { return (size_t)v.n; };
    auto nNode = [](const amos_bow_view &v) { return (size_t)v.n_nodes; };
    amos_bow_search s;
    s.d_kps = (const amos_keypoint *)both(cap, sizeof(amos_keypoint), [](const amos_bow_view &v) { return (const void *)v.keys; }, nFeat);
    s.d_desc = both(cap, 32, [](const amos_bow_view &v) { return (const void *)v.descriptors; }, nFeat);
    s.d_node_ids = (const uint32_t *)both(cap, 4, [](const amos_bow_view &v) { return (const void *)v.node_ids; }, nNode);
    s.d_node_off = (const int32_t *)both(cap + 1, 4, [](const amos_bow_view &v) { return (const void *)v.node_off; },
                                         [](const amos_bow_view &v) { return v.n_nodes ? (size_t)v.n_nodes + 1 : 0; });
    s.d_node_idx = (const int32_t *)both(cap, 4, [](const amos_bow_view &v) { return (const void *)v.node_idx; },
                                         [](const amos_bow_view &v) { return v.n_nodes ? (size_t)v.node_off[v.n_nodes] : 0; });
    s.d_has_point = kf->has_point ? both(cap, 1, [](const amos_bow_view &v) { return (const void *)v.has_point; }, nFeat) : nullptr;
    const int32_t counts[2] = {kf->n, f->n}, nodes[2] = {kf->n_nodes, f->n_nodes}, slots[2] = {0, 1};
    s.d_counts = stage_input<int32_t>(m, counts, sizeof(counts));
    s.d_n_nodes = stage_input<int32_t>(m, nodes, sizeof(nodes));
    s.d_pairs_kf = stage_input<int32_t>(m, slots, sizeof(slots));
    s.d_pairs_f = s.d_pairs_kf + 1;
    uint8_t *out = (uint8_t *)m->dOut;
    s.d_match = (int32_t *)out; s.d_stats = (amos_bow_search_stats *)(out + bytesMatch);
    s.n_pairs = 1; s.capacity = (int32_t)cap; s.nn_ratio = nn_ratio; s.check_orientation = check_orientation;
    if ((rc = stage_flush(m)) != AMOS_OK || (rc = amos_match_bow_batch_device(m, &s)) != AMOS_OK) return rc;
    const uint8_t *h = m->hStage + stage_take(m, bytesOut);
    AMOS_HIP_CHECK(hipMemcpyAsync((void *)h, out, bytesOut, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (f->n) std::memcpy(matches_f, h, sizeof(int32_t) * (size_t)f->n);
    std::memcpy(stats, h + bytesMatch, sizeof(*stats));
    return AMOS_OK;
}

}  // extern "C"
