// amos_bow.hip -- Frame::ComputeBoW (Frame.cc:1033-1049) for a batch of resident frames: DBoW2's TemplatedVocabulary::transform(features,
// BowVector&, FeatureVector&, levelsup) (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259) over a vocabulary tree that lives on the
// device.
//
// Launches on the handle's stream: k_bow_descend (sixteen lanes per feature walk the tree: one child each, a second round for nodes with
// 17 .. 32 children) and k_bow_vectors (one work-group per frame: a sort of (node id, feature) keys in LDS gives the FeatureVector as CSR, a
// sort of (word id, feature) keys the BowVector, whose values are summed and normalised in the reference's order).  The arithmetic is
// defined in include/amos_frontend.h, "bag of words".
#include "amos_block.h"
#include "amos_projection_search.h"  // Desc, grow, align64

#include <vector>

namespace amos {

static_assert(sizeof(amos_bow_stats) == 16, "amos_bow_stats is 16 bytes (include/amos_frontend.h)");

// One node of the tree at its POSITION: the children of a node sit side by side, in ascending node id (position 0 is the root).
struct BowNode {
    int nodeId;
    int childBegin;  // position of the first child
    int nChildren;   // 0: a leaf
    uint32_t word;   // a leaf's word id
};

constexpr int kBowLanes = 16;      // lanes per feature of the descent
constexpr int kBowThreads = 256;   // work-group of k_bow_vectors
constexpr unsigned long long kNoKey = ~0ull;

struct BowArgs {
    const BowNode *nodes;    // by position
    const uint8_t *desc;     // by position, 32 bytes each
    const double *weight;    // by position
    const int *depth;        // by NODE ID: the root 0, its children 1, ...
    const uint8_t *features; // [frames][capacity][32]
    const int *counts;
    uint32_t *featWord, *featNode;
    int *nNodes, *nodeOff, *nodeIdx, *nWords;
    uint32_t *nodeIds, *words;
    double *wordWeights;
    amos_bow_stats *stats;
    int *featPos;            // scratch [frames][capacity]: the position of the feature's leaf
    int capacity, nidLevel, sortCap;  // nidLevel = L - levelsup; sortCap: capacity rounded up to a power of two
};

// ---- the descent of TemplatedVocabulary.h:1218-1259.  grid = (ceil(capacity / 16), frames), block = 256: sixteen features.
// The lanes of a feature stay together (what they branch on is the same in all sixteen); the loop itself runs until every feature of the
// wave is at its leaf, so the group reductions are reached by whole waves.
__global__ __launch_bounds__(256) void k_bow_descend(const BowArgs a)
{
    const int f = blockIdx.y, sub = threadIdx.x % kBowLanes;
    const int i = blockIdx.x * (256 / kBowLanes) + threadIdx.x / kBowLanes;
    const int n = min(max(a.counts[f], 0), a.capacity);
    bool done = i >= n;
    Desc d = {};
    if (!done) d = load_desc(a.features + ((size_t)f * a.capacity + i) * 32);
    int pos = 0, level = 0;
    uint32_t nid = 0;  // the root: stands when L - levelsup <= 0
    BowNode cur = a.nodes[0];
    while (__any(!done)) {
        unsigned key = 0xffffffffu;
        if (!done) {
#pragma unroll
            for (int c0 = 0; c0 < AMOS_BOW_MAX_CHILDREN; c0 += kBowLanes) {
                const int c = c0 + sub;
                if (c < cur.nChildren) {
                    const int dist = hamming256(d, load_desc(a.desc + (size_t)(cur.childBegin + c) * 32));
                    key = min(key, ((unsigned)dist << 8) | (unsigned)c);  // the first child of equal distances
                }
            }
        }
#pragma unroll
        for (int off = kBowLanes / 2; off > 0; off >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, off, kBowLanes));
        if (!done) {
            pos = cur.childBegin + (int)(key & 0xffu);
            cur = a.nodes[pos];
            level++;
            if (level == a.nidLevel) nid = (uint32_t)cur.nodeId;
            if (cur.nChildren == 0) {
                if (level < a.nidLevel) nid = (uint32_t)cur.nodeId;  // a leaf above the level: see the header
                done = true;
            }
        }
    }
    if (i < n && sub == 0) {
        const size_t o = (size_t)f * a.capacity + i;
        a.featWord[o] = a.weight[pos] > 0 ? cur.word : AMOS_BOW_NO_WORD;
        a.featNode[o] = nid;
        a.featPos[o] = pos;
    }
}

// sorted keys (id << 32 | feature) in LDS, m of them -> the CSR of their ids: ids[c], off[c] for the c-th distinct id, idx[j] the features;
// perHead(c, j) for each segment's first position.  Returns the number of ids.  Every thread of the group calls.
template <class PerHead>
__device__ __forceinline__ int csr_of_sorted(const unsigned long long *keys, int m, int *sWave, PerHead perHead)
{
    return block_compact<kBowThreads>(m, sWave, [&](int j) { return j == 0 || (keys[j] >> 32) != (keys[j - 1] >> 32); },
                                      [&](int j, int c) { if (c >= 0) perHead(c, j); });
}

// ---- TemplatedVocabulary.h:1145-1193 for one frame per work-group.  grid = frames, block = 256, dynamic LDS = sortCap keys + the
// per-wave counts of the compaction.
__global__ __launch_bounds__(kBowThreads) void k_bow_vectors(const BowArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);
    int *sWave = reinterpret_cast<int *>(smem + (size_t)a.sortCap * 8);
    const int f = blockIdx.x, t = threadIdx.x;
    const int n = min(max(a.counts[f], 0), a.capacity);
    const size_t o = (size_t)f * a.capacity;
    int sortN = 1;
    while (sortN < n) sortN <<= 1;  // <= sortCap

    // the FeatureVector: keys (nid, feature) of the features that are not stopped
    int stopped = 0, early = 0;
    for (int i = t; i < sortN; i += kBowThreads) {
        unsigned long long key = kNoKey;
        if (i < n) {
            const uint32_t nid = a.featNode[o + i];
            early |= a.nidLevel > 0 && a.depth[nid] < a.nidLevel;
            if (a.featWord[o + i] != AMOS_BOW_NO_WORD) key = ((unsigned long long)nid << 32) | (unsigned)i;
            else stopped++;
        }
        keys[i] = key;
    }
    const int nStopped = block_sum<kBowThreads>(stopped, sWave);
    const int anyEarly = block_sum<kBowThreads>(early, sWave);
    const int m = n - nStopped;  // the sorted keys' first m are the features that count
    block_sort_u64<kBowThreads>(keys, sortN);
    const int nNodes = csr_of_sorted(keys, m, sWave, [&](int c, int j) {
        a.nodeIds[o + c] = (uint32_t)(keys[j] >> 32);
        a.nodeOff[(size_t)f * (a.capacity + 1) + c] = j;
    });
    for (int j = t; j < m; j += kBowThreads) a.nodeIdx[o + j] = (int)(keys[j] & 0xffffffffu);
    if (t == 0) a.nodeOff[(size_t)f * (a.capacity + 1) + nNodes] = m;
    __syncthreads();

    // the BowVector: keys (word, feature); a word's value is its weight added once per feature, in feature order, from the first weight
    for (int i = t; i < sortN; i += kBowThreads) {
        unsigned long long key = kNoKey;
        if (i < n) {
            const uint32_t w = a.featWord[o + i];
            if (w != AMOS_BOW_NO_WORD) key = ((unsigned long long)w << 32) | (unsigned)i;
        }
        keys[i] = key;
    }
    block_sort_u64<kBowThreads>(keys, sortN);
    const int nWords = csr_of_sorted(keys, m, sWave, [&](int c, int j) {
        const unsigned long long id = keys[j] >> 32;
        double v = a.weight[a.featPos[o + (keys[j] & 0xffffffffu)]];
        for (int e = j + 1; e < m && (keys[e] >> 32) == id; e++) v = __dadd_rn(v, a.weight[a.featPos[o + (keys[e] & 0xffffffffu)]]);
        a.words[o + c] = (uint32_t)id;
        a.wordWeights[o + c] = v;
    });
    __threadfence_block();
    __syncthreads();  // the values are written before one lane sums them
    // BowVector::normalize(L1) (BowVector.cpp:62-84): one addition per word, in word order
    double *sNorm = reinterpret_cast<double *>(keys);
    if (t == 0) {
        double norm = 0.0;
        for (int c = 0; c < nWords; c++) norm = __dadd_rn(norm, fabs(a.wordWeights[o + c]));
        sNorm[0] = norm;
    }
    __syncthreads();
    const double norm = sNorm[0];
    if (norm > 0.0)
        for (int c = t; c < nWords; c += kBowThreads) a.wordWeights[o + c] = __ddiv_rn(a.wordWeights[o + c], norm);
    if (t == 0) {
        a.nNodes[f] = nNodes;
        a.nWords[f] = nWords;
        amos_bow_stats s;
        s.n_words = nWords; s.n_nodes = nNodes; s.n_stopped = nStopped; s.status = anyEarly ? AMOS_BOW_STATUS_EARLY_LEAF : 0;
        a.stats[f] = s;
    }
}

static DeviceOnce g_vectorsLds;

// the children lists and the checks of amos_bow_create; children[p] in ascending node id
static int bow_check(const char *name, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent, const uint8_t *is_leaf,
                     std::vector<std::vector<int>> *children, int32_t *n_words)
{
    (void)k;  // the file's branching factor sizes nothing here: a node has the children that name it
    if (!parent || !is_leaf || n_nodes < 2) { set_error("%s: invalid argument", name); return AMOS_ERR_INVALID; }
    if (scoring != AMOS_BOW_L1_NORM || weighting != AMOS_BOW_TF_IDF) {
        set_error("%s: scoring %d / weighting %d: only L1_NORM (0) / TF_IDF (0) are built", name, scoring, weighting);
        return AMOS_ERR_INVALID;
    }
    if (L < 1 || L > 10) { set_error("%s: L = %d outside 1 .. 10", name, L); return AMOS_ERR_INVALID; }
    std::vector<std::vector<int>> ch((size_t)n_nodes);
    for (int i = 1; i < n_nodes; i++) {
        if (parent[i] < 0 || parent[i] >= i) { set_error("%s: parent[%d] = %d is not an earlier node", name, i, parent[i]); return AMOS_ERR_INVALID; }
        ch[parent[i]].push_back(i);
    }
    int words = 0;
    for (int i = 0; i < n_nodes; i++) {
        const bool leaf = i > 0 && is_leaf[i] != 0;
        if (leaf != ch[i].empty()) {
            set_error("%s: node %d is %s", name, i, leaf ? "a leaf with children" : "no leaf and has no children");
            return AMOS_ERR_INVALID;
        }
        if (ch[i].size() > AMOS_BOW_MAX_CHILDREN) { set_error("%s: node %d has %zu children (at most %d)", name, i, ch[i].size(), AMOS_BOW_MAX_CHILDREN); return AMOS_ERR_INVALID; }
        words += leaf;
    }
    if (n_words) *n_words = words;
    if (children) children->swap(ch);
    return AMOS_OK;
}

}  // namespace amos

struct amos_bow : amos::StreamHandle {
    int k = 0, L = 0, nNodes = 0, nWords = 0;
    amos::BowNode *dNodes = nullptr;
    uint8_t *dDesc = nullptr;
    double *dWeight = nullptr;
    int *dDepth = nullptr;
    int *dFeatPos = nullptr;   // scratch of the call in flight (calls are ordered on the stream)
    size_t capFeatPos = 0;
    uint8_t *dFrame = nullptr, *hFrame = nullptr;  // the host form's one frame: inputs and outputs, device and pinned
    size_t capFrame = 0;
};

using namespace amos;

extern "C" {

int amos_bow_check(int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent, const uint8_t *is_leaf, int32_t *n_words)
{
    return bow_check("amos_bow_check", k, L, scoring, weighting, n_nodes, parent, is_leaf, nullptr, n_words);
}

int amos_bow_create(int device, void *stream, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent,
                    const uint8_t *is_leaf, const uint8_t *desc, const double *weight, amos_bow **out)
{
    if (!out || !desc || !weight) { set_error("amos_bow_create: invalid argument"); return AMOS_ERR_INVALID; }
    std::vector<std::vector<int>> children;
    int32_t nWords = 0;
    int rc = bow_check("amos_bow_create", k, L, scoring, weighting, n_nodes, parent, is_leaf, &children, &nWords);
    if (rc != AMOS_OK) return rc;
    // positions: the root, then every node's children side by side, parents in ascending node id (parent[i] < i: a node has its position
    // before its children are placed)
    std::vector<int> posOf((size_t)n_nodes, 0), depth((size_t)n_nodes, 0);
    std::vector<BowNode> nodes((size_t)n_nodes);
    std::vector<uint8_t> hDesc((size_t)n_nodes * 32, 0);
    std::vector<double> hWeight((size_t)n_nodes, 0.0);
    std::vector<uint32_t> wordOf((size_t)n_nodes, 0);
    uint32_t w = 0;
    for (int i = 1; i < n_nodes; i++) if (is_leaf[i]) wordOf[i] = w++;
    int next = 1;
    for (int i = 0; i < n_nodes; i++) {
        BowNode &nd = nodes[posOf[i]];
        nd.nodeId = i; nd.childBegin = next; nd.nChildren = (int)children[i].size(); nd.word = wordOf[i];
        for (int c : children[i]) {
            posOf[c] = next++;
            depth[c] = depth[i] + 1;
        }
        if (i > 0) {
            std::memcpy(&hDesc[(size_t)posOf[i] * 32], desc + (size_t)i * 32, 32);
            hWeight[posOf[i]] = weight[i];
        }
    }
    amos_bow *b = new amos_bow();
    rc = b->open(device, stream);
    if (rc != AMOS_OK) { delete b; return rc; }
    b->k = k; b->L = L; b->nNodes = n_nodes; b->nWords = nWords;
    const size_t nn = (size_t)n_nodes;
    if (hipMalloc((void **)&b->dNodes, nn * sizeof(BowNode)) != hipSuccess || hipMalloc((void **)&b->dDesc, nn * 32) != hipSuccess ||
        hipMalloc((void **)&b->dWeight, nn * sizeof(double)) != hipSuccess || hipMalloc((void **)&b->dDepth, nn * sizeof(int)) != hipSuccess ||
        hipMemcpy(b->dNodes, nodes.data(), nn * sizeof(BowNode), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->dDesc, hDesc.data(), nn * 32, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->dWeight, hWeight.data(), nn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->dDepth, depth.data(), nn * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        set_error("amos_bow_create: the vocabulary of %d nodes could not be placed on the device", n_nodes);
        amos_bow_destroy(b);
        return AMOS_ERR_DEVICE;
    }
    *out = b;
    return AMOS_OK;
}

void amos_bow_destroy(amos_bow *b)
{
    if (!b) return;
    b->close();
    void *ptrs[] = {b->dNodes, b->dDesc, b->dWeight, b->dDepth, b->dFeatPos, b->dFrame};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (b->hFrame) (void)hipHostFree(b->hFrame);
    delete b;
}

int amos_bow_sync(amos_bow *b)
{
    if (!b) return AMOS_ERR_INVALID;
    AMOS_HIP_CHECK(hipStreamSynchronize(b->stream));
    return AMOS_OK;
}

void *amos_bow_stream(amos_bow *b) { return b ? (void *)b->stream : nullptr; }

int amos_bow_transform_batch_device(amos_bow *b, const uint8_t *d_desc, const int32_t *d_counts, int n_frames, int capacity, int levelsup,
                                    uint32_t *d_feat_word, uint32_t *d_feat_node, int32_t *d_n_nodes, uint32_t *d_node_ids,
                                    int32_t *d_node_off, int32_t *d_node_idx, int32_t *d_n_words, uint32_t *d_words,
                                    double *d_word_weights, amos_bow_stats *d_stats)
{
    if (!b || !d_desc || !d_counts || n_frames < 1 || capacity < 1 || levelsup < 0 || !d_feat_word || !d_feat_node || !d_n_nodes ||
        !d_node_ids || !d_node_off || !d_node_idx || !d_n_words || !d_words || !d_word_weights || !d_stats) {
        set_error("amos_bow_transform_batch_device: invalid argument");
        return AMOS_ERR_INVALID;
    }
    if (capacity > AMOS_BOW_MAX_CAPACITY) {
        set_error("amos_bow_transform_batch_device: capacity %d above %d (the sort keys of a frame live in LDS)", capacity, AMOS_BOW_MAX_CAPACITY);
        return AMOS_ERR_CAPACITY;
    }
    AMOS_HIP_CHECK(hipSetDevice(b->device));
    int rc = grow(&b->dFeatPos, &b->capFeatPos, (size_t)n_frames * capacity);
    if (rc != AMOS_OK) return rc;
    BowArgs a;
    a.nodes = b->dNodes; a.desc = b->dDesc; a.weight = b->dWeight; a.depth = b->dDepth;
    a.features = d_desc; a.counts = d_counts;
    a.featWord = d_feat_word; a.featNode = d_feat_node;
    a.nNodes = d_n_nodes; a.nodeOff = d_node_off; a.nodeIdx = d_node_idx; a.nWords = d_n_words;
    a.nodeIds = d_node_ids; a.words = d_words; a.wordWeights = d_word_weights; a.stats = d_stats;
    a.featPos = b->dFeatPos;
    a.capacity = capacity; a.nidLevel = b->L - levelsup;
    a.sortCap = 1;
    while (a.sortCap < capacity) a.sortCap <<= 1;
    const int ldsBytes = a.sortCap * 8 + 64;  // + the compaction's per-wave counts (and the norm's slot lies in the keys)
    AMOS_HIP_CHECK(set_max_dynamic_lds(g_vectorsLds, (const void *)k_bow_vectors, AMOS_BOW_MAX_CAPACITY * 8 + 64, b->stream));
    hipLaunchKernelGGL(k_bow_descend, dim3((capacity + 256 / kBowLanes - 1) / (256 / kBowLanes), n_frames), dim3(256), 0, b->stream, a);
    hipLaunchKernelGGL(k_bow_vectors, dim3(n_frames), dim3(kBowThreads), ldsBytes, b->stream, a);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_bow_transform(amos_bow *b, const uint8_t *desc, int n, int levelsup, uint32_t *feat_word, uint32_t *feat_node, uint32_t *node_ids,
                       int32_t *node_off, int32_t *node_idx, uint32_t *words, double *word_weights, amos_bow_stats *stats)
{
    if (!b || n < 0 || levelsup < 0 || !stats || !node_off ||
        (n > 0 && (!desc || !feat_word || !feat_node || !node_ids || !node_idx || !words || !word_weights))) {
        set_error("amos_bow_transform: invalid argument");
        return AMOS_ERR_INVALID;
    }
    if (n > AMOS_BOW_MAX_CAPACITY) { set_error("amos_bow_transform: %d features above %d", n, AMOS_BOW_MAX_CAPACITY); return AMOS_ERR_CAPACITY; }
    AMOS_HIP_CHECK(hipSetDevice(b->device));
    const size_t cap = (size_t)std::max(n, 1);
    // one buffer: the inputs (descriptors, count), then the outputs in download order
    const size_t oCount = align64(cap * 32), oOut = oCount + 64, oWeights = oOut, oStats = oWeights + align64(cap * 8), oNNodes = oStats + 64,
                 oNWords = oNNodes + 64, oFeatWord = oNWords + 64, oFeatNode = oFeatWord + align64(cap * 4), oNodeIds = oFeatNode + align64(cap * 4),
                 oNodeOff = oNodeIds + align64(cap * 4), oNodeIdx = oNodeOff + align64((cap + 1) * 4), oWords = oNodeIdx + align64(cap * 4),
                 oEnd = oWords + align64(cap * 4);
    if (oEnd > b->capFrame) {
        (void)hipStreamSynchronize(b->stream);
        if (b->dFrame) (void)hipFree(b->dFrame);
        if (b->hFrame) (void)hipHostFree(b->hFrame);
        b->dFrame = b->hFrame = nullptr;
        b->capFrame = 0;
        const size_t bytes = oEnd + oEnd / 2;
        if (hipMalloc((void **)&b->dFrame, bytes) != hipSuccess || hipHostMalloc((void **)&b->hFrame, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            set_error("amos_bow_transform: %zu bytes (pinned host + device) could not be allocated", bytes);
            return AMOS_ERR_DEVICE;
        }
        b->capFrame = bytes;
    }
    if (n) std::memcpy(b->hFrame, desc, (size_t)n * 32);
    *reinterpret_cast<int32_t *>(b->hFrame + oCount) = n;
    AMOS_HIP_CHECK(hipMemcpyAsync(b->dFrame, b->hFrame, oOut, hipMemcpyHostToDevice, b->stream));
    uint8_t *d = b->dFrame;
    const int rc = amos_bow_transform_batch_device(b, d, (const int32_t *)(d + oCount), 1, (int)cap, levelsup, (uint32_t *)(d + oFeatWord),
                                                   (uint32_t *)(d + oFeatNode), (int32_t *)(d + oNNodes), (uint32_t *)(d + oNodeIds),
                                                   (int32_t *)(d + oNodeOff), (int32_t *)(d + oNodeIdx), (int32_t *)(d + oNWords),
                                                   (uint32_t *)(d + oWords), (double *)(d + oWeights), (amos_bow_stats *)(d + oStats));
    if (rc != AMOS_OK) return rc;
    AMOS_HIP_CHECK(hipMemcpyAsync(b->hFrame + oOut, d + oOut, oEnd - oOut, hipMemcpyDeviceToHost, b->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(b->stream));
    const uint8_t *h = b->hFrame;
    const amos_bow_stats s = *reinterpret_cast<const amos_bow_stats *>(h + oStats);
    *stats = s;
    if (n) {
        std::memcpy(feat_word, h + oFeatWord, (size_t)n * 4);
        std::memcpy(feat_node, h + oFeatNode, (size_t)n * 4);
        std::memcpy(node_ids, h + oNodeIds, (size_t)s.n_nodes * 4);
        std::memcpy(node_idx, h + oNodeIdx, (size_t)(n - s.n_stopped) * 4);
        std::memcpy(words, h + oWords, (size_t)s.n_words * 4);
        std::memcpy(word_weights, h + oWeights, (size_t)s.n_words * 8);
    }
    std::memcpy(node_off, h + oNodeOff, (size_t)(s.n_nodes + 1) * 4);
    return AMOS_OK;
}

}  // extern "C"
