"""DBoW2's TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259,
BowVector.cpp:34-46, 62-84, FeatureVector.cpp) and ORBmatcher::SearchByBoW(pKF, F, ...) (ORBmatcher.cc:230-382), restated loop by loop in plain
Python (dicts and lists, Python floats are IEEE doubles), and a generator of synthetic vocabularies.  Independent of the device code: the
tests hold the device to it, and test_bow_cpu.py holds IT to numpy properties."""
import numpy as np

NO_WORD = 0xFFFFFFFF
TH_LOW, HISTO_LENGTH = 50, 30

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


class Vocabulary:
    """What loadFromTextFile (TemplatedVocabulary.h:1338-1424) builds: node 0 is the root; nodes 1 .. n - 1 in file order."""

    def __init__(self, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0):
        self.k, self.L, self.scoring, self.weighting = k, L, scoring, weighting
        self.parent = np.asarray(parent, np.int32)
        self.is_leaf = np.asarray(is_leaf, np.uint8)
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.weight = np.asarray(weight, np.float64)
        n = len(self.parent)
        self.children = [[] for _ in range(n)]
        self.word_id = [None] * n
        words = 0
        for nid in range(1, n):  # :1378-1420
            self.children[int(self.parent[nid])].append(nid)
            if self.is_leaf[nid] > 0:
                self.word_id[nid] = words
                words += 1
        self.n_words = words

    @property
    def n_nodes(self):
        return len(self.parent)

    def arrays(self):
        return self.parent, self.is_leaf, self.desc, self.weight

    def to_text(self):
        """ORBvoc.txt's format: 'k L scoring weighting', then per node 'parent is_leaf 32 bytes weight'."""
        lines = [f"{self.k} {self.L} {self.scoring} {self.weighting}"]
        for nid in range(1, self.n_nodes):
            lines.append(f"{int(self.parent[nid])} {int(self.is_leaf[nid])} " + " ".join(str(int(b)) for b in self.desc[nid]) + f" {float(self.weight[nid])!r}")
        return "\n".join(lines) + "\n"


def transform_feature(voc, feature, levelsup):
    """:1218-1259 -> (word id, weight, nid, early, path): early is set where the reference leaves nid uninitialised (the walk ends at a leaf
    above level L - levelsup; nid is then DEFINED as that leaf); path lists, per level, (children, their distances, the chosen child)."""
    nid_level = voc.L - levelsup
    nid = 0 if nid_level <= 0 else None
    final_id, current_level, path = 0, 0, []
    while True:
        current_level += 1
        nodes = voc.children[final_id]
        final_id = nodes[0]
        best_d = hamming(feature, voc.desc[final_id])
        dists = [best_d]
        for cid in nodes[1:]:
            d = hamming(feature, voc.desc[cid])
            dists.append(d)
            if d < best_d:
                best_d, final_id = d, cid
        path.append((list(nodes), dists, final_id))
        if current_level == nid_level:
            nid = final_id
        if voc.is_leaf[final_id] > 0:
            break
    early = nid is None
    if early:
        nid = final_id
    return voc.word_id[final_id], float(voc.weight[final_id]), nid, early, path


def transform(voc, features, levelsup):
    """:1127-1194 for TF_IDF / L1_NORM.  Returns a dict: feat_word, feat_node (per feature), bow (word -> value, insertion = ascending after the
    sort below), fv (node -> [features]), and the flat arrays of the C ABI."""
    features = np.asarray(features, np.uint8).reshape(-1, 32)
    v, fv = {}, {}
    feat_word, feat_node, status, stopped = [], [], 0, 0
    for i_feature, f in enumerate(features):
        wid, w, nid, early, _ = transform_feature(voc, f, levelsup)
        status |= 1 if early else 0
        feat_node.append(nid)
        if w > 0:  # not stopped
            if wid in v:
                v[wid] += w  # BowVector::addWeight
            else:
                v[wid] = w
            fv.setdefault(nid, []).append(i_feature)  # FeatureVector::addFeature
            feat_word.append(wid)
        else:
            feat_word.append(NO_WORD)
            stopped += 1
    words = sorted(v)  # a std::map iterates in ascending key order
    norm = 0.0
    for wid in words:  # BowVector::normalize(L1)
        norm += abs(v[wid])
    if norm > 0.0:
        for wid in words:
            v[wid] /= norm
    node_ids = sorted(fv)
    node_off, node_idx = [0], []
    for nid in node_ids:
        node_idx.extend(fv[nid])
        node_off.append(len(node_idx))
    return {"feat_word": np.array(feat_word, np.uint32), "feat_node": np.array(feat_node, np.uint32),
            "bow": {w: v[w] for w in words}, "fv": {n: fv[n] for n in node_ids},
            "node_ids": np.array(node_ids, np.uint32), "node_off": np.array(node_off, np.int32), "node_idx": np.array(node_idx, np.int32),
            "words": np.array(words, np.uint32), "word_weights": np.array([v[w] for w in words], np.float64),
            "stats": {"n_words": len(words), "n_nodes": len(node_ids), "n_stopped": stopped, "status": status}}


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1866-1908)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def search_by_bow(kf, f, nn_ratio, check_orientation):
    """ORBmatcher.cc:230-382 on two dicts (angles, desc, fv: node -> [features]; kf also has_point or None).  Returns (matches_f, stats): the
    reference's result plus what the device form counts: n_queries (keyframe features that reach the candidate loop) and n_researched (those
    whose best or second best over ALL features of the node, the first of equal distances each, is already matched at their turn)."""
    n_f = len(f["desc"])
    matches = [-1] * n_f
    hist = [[] for _ in range(HISTO_LENGTH)]
    factor = np.float32(HISTO_LENGTH) / np.float32(360.0)
    nmatches = n_queries = n_researched = 0
    nn_ratio = np.float32(nn_ratio)
    for node in sorted(kf["fv"]):
        if node not in f["fv"]:
            continue
        for real_kf in kf["fv"][node]:
            if kf.get("has_point") is not None and not kf["has_point"][real_kf]:
                continue
            n_queries += 1
            d_kf = kf["desc"][real_kf]
            best1, best_idx, best2 = 256, -1, 256
            free = []  # (dist, feature) of ALL candidates, for the unrestricted best two
            dists = _POP[np.bitwise_xor(f["desc"][f["fv"][node]], d_kf[None, :])].sum(1)  # DescriptorDistance to every candidate
            for real_f, dist in zip(f["fv"][node], dists.tolist()):
                free.append((dist, real_f))
                if matches[real_f] >= 0:
                    continue
                if dist < best1:
                    best2, best1, best_idx = best1, dist, real_f
                elif dist < best2:
                    best2 = dist
            top = sorted((c for c in free if c[0] < 256), key=lambda c: c[0])[:2]  # stable: the first of equal distances
            if any(matches[c[1]] >= 0 for c in top):
                n_researched += 1
            if best1 <= TH_LOW and np.float32(best1) < nn_ratio * np.float32(best2):
                matches[best_idx] = real_kf
                if check_orientation:
                    rot = np.float32(kf["angles"][real_kf]) - np.float32(f["angles"][best_idx])
                    if rot < 0.0:
                        rot = np.float32(rot + np.float32(360.0))
                    b = int(np.floor(float(np.float32(rot * factor)) + 0.5))  # C round() of a value >= 0: half away from zero
                    if b == HISTO_LENGTH:
                        b = 0
                    hist[b].append(best_idx)
                nmatches += 1
    if check_orientation:
        ind = three_maxima([len(h) for h in hist])
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for j in hist[i]:
                matches[j] = -1
                nmatches -= 1
    return np.array(matches, np.int32), {"n_queries": n_queries, "n_matches": nmatches, "n_researched": n_researched}


# ---------------------------------------------------------------------------------------------------------------- synthetic vocabularies

def make_vocabulary(k, L, seed, flips=40, duplicate_share=0.0, bad_weight_share=0.15, irregular=False, all_stopped=False):
    """A tree of depth L: a child's descriptor is its parent's with `flips` random bits flipped; with duplicate_share some children copy their
    elder sibling exactly (ties); a share of the leaves gets a zero or negative weight (stopped words); irregular: 1 .. k children per node
    and leaves above level L."""
    rng = np.random.default_rng(seed)
    parent, is_leaf, desc, weight, level = [0], [0], [rng.integers(0, 256, 32, dtype=np.uint8)], [0.0], [0]
    frontier = [0]
    while frontier:
        nxt = []
        for p in frontier:
            n_children = int(rng.integers(1, k + 1)) if irregular and p > 0 else k  # (the root keeps k: the tree stays bushy)
            for c in range(n_children):
                nid = len(parent)
                d = desc[p].copy()
                if c > 0 and rng.random() < duplicate_share:
                    d = desc[nid - 1].copy()
                else:
                    bits = rng.choice(256, size=flips, replace=False)
                    for b in bits:
                        d[b >> 3] ^= np.uint8(1 << (b & 7))
                lvl = level[p] + 1
                leaf = lvl == L or (irregular and lvl >= 1 and rng.random() < 0.25)
                parent.append(p); is_leaf.append(1 if leaf else 0); desc.append(d); level.append(lvl)
                if leaf:
                    r = rng.random()
                    w = float(rng.uniform(0.05, 9.0))
                    if all_stopped or r < bad_weight_share:
                        w = 0.0 if (r * 1000) % 2 < 1 else -w
                    weight.append(w)
                else:
                    weight.append(0.0)
                    nxt.append(nid)
        frontier = nxt
    return Vocabulary(k, L, parent, is_leaf, np.array(desc, np.uint8), weight)


def make_features(voc, n, seed, flips=25):
    """n descriptors near random nodes of the vocabulary (so that the walks spread over the tree), some of them exact node descriptors."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        d = voc.desc[int(rng.integers(1, voc.n_nodes))].copy()
        if rng.random() > 0.1:
            for b in rng.choice(256, size=flips, replace=False):
                d[b >> 3] ^= np.uint8(1 << (b & 7))
        out[i] = d
    return out
