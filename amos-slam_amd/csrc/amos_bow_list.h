// amos_bow_list.h -- what the searches over two FeatureVectors (amos_bow_search.hip) are built on: one frame's side of the resident CSR
// with its clamps, the wave-wide search of one node's list, and what a host form asks of an amos_bow_view before its arrays go to the
// device.
#pragma once
#include "amos_projection_search.h"  // TakenBitmap, best-two keys, the matcher's staging

#include "../../include/amos_host_types.h"  // amos_bow_view

namespace amos {

// one frame's FeatureVector and features; whatever is read of the arrays is clamped into them
struct BowSide {
    int n, nNodes;
    const uint32_t *ids;
    const int *off, *idx;
    const uint8_t *desc;
    const amos_keypoint *kps;
};
// A: the arguments of a search (kps, desc, counts, nNodes, nodeIds, nodeOff, nodeIdx, capacity)
template <class A>
__device__ __forceinline__ BowSide bow_side(const A &a, int slot)
{
    const size_t o = (size_t)slot * a.capacity;
    BowSide s;
    s.n = min(max(a.counts[slot], 0), a.capacity);
    s.nNodes = min(max(a.nNodes[slot], 0), a.capacity);
    s.ids = a.nodeIds + o; s.off = a.nodeOff + (size_t)slot * (a.capacity + 1); s.idx = a.nodeIdx + o;
    s.desc = a.desc + o * 32; s.kps = a.kps + o;
    return s;
}
template <class A>
__device__ __forceinline__ int bow_off(const A &a, const BowSide &s, int node) { return min(max(s.off[node], 0), a.capacity); }

// The whole wave searches the list positions [b0, b1) of a node; cand(j) gives the key of position j (unique per position, the smaller
// the better) or 0xffffffff when it holds no candidate: pushing that changes nothing, so the loop keeps no flag beside the two keys.  All
// 64 lanes call it converged; best / second come back wave-uniform, 0xffffffff for none.
template <class Cand>
__device__ __forceinline__ void wave_list_keys(int b0, int b1, int lane, Cand cand, unsigned &best, unsigned &second)
{
    best = second = 0xffffffffu;
    for (int j = b0 + lane; j < b1; j += 64) top2_push(best, second, cand(j));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned ob = __shfl_xor(best, off, 64), os = __shfl_xor(second, off, 64);
        top2_merge(best, second, ob, os);
    }
    best = __builtin_amdgcn_readfirstlane(best);
    second = __builtin_amdgcn_readfirstlane(second);
}

// what a host form asks of a view before its arrays go to the device
inline bool bow_view_ok(const amos_bow_view *v)
{
    if (!v || v->n < 0 || v->n > 65536 || v->n_nodes < 0 || v->n_nodes > std::max(v->n, 1)) return false;
    if (v->n > 0 && (!v->keys || !v->descriptors)) return false;
    if (v->n_nodes == 0) return true;
    if (!v->node_ids || !v->node_off || !v->node_idx || v->node_off[0] != 0) return false;
    for (int i = 0; i < v->n_nodes; i++) {
        if (v->node_off[i + 1] < v->node_off[i] || (i > 0 && v->node_ids[i] <= v->node_ids[i - 1])) return false;
    }
    if (v->node_off[v->n_nodes] > v->n) return false;
    for (int j = 0; j < v->node_off[v->n_nodes]; j++) if (v->node_idx[j] < 0 || v->node_idx[j] >= v->n) return false;
    return true;
}

}  // namespace amos
