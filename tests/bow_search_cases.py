"""Inputs of the SearchByBoW tests, and orc_search_by_bow (oracle/orb_oracle.c) bound for them.  A side of a search is a dict: keys (KP_DTYPE),
angles, desc [n][32], fv (node id -> [feature indices], a DBoW2::FeatureVector) and, for a keyframe, has_point (uint8 [n]) or None."""
import ctypes as C

import numpy as np

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class BowView(C.Structure):
    """amos_bow_view (include/amos_host_types.h)."""
    _fields_ = [("n", C.c_int32), ("keys", C.c_void_p), ("descriptors", C.c_void_p), ("has_point", C.c_void_p), ("u_right", C.c_void_p),
                ("n_nodes", C.c_int32), ("node_ids", C.c_void_p), ("node_off", C.c_void_p), ("node_idx", C.c_void_p)]


def side(desc, angles, fv, has_point=None):
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    keys = np.zeros(len(desc), KP)
    keys["angle"] = np.asarray(angles, np.float32)
    hp = None if has_point is None else np.ascontiguousarray(has_point, np.uint8)
    return {"keys": keys, "angles": keys["angle"].copy(), "desc": desc, "fv": {int(k): [int(i) for i in v] for k, v in fv.items()}, "has_point": hp}


def csr(fv):
    """node id -> [features] as the flat arrays of amos_bow_view: (node_ids, node_off, node_idx)"""
    ids = np.array(sorted(fv), np.uint32)
    off, idx = [0], []
    for nid in ids:
        idx.extend(fv[int(nid)])
        off.append(len(idx))
    return ids, np.array(off, np.int32), np.array(idx, np.int32)


def with_csr(s):
    ids, off, idx = csr(s["fv"])
    return dict(s, node_ids=ids, node_off=off, node_idx=idx)


def _view(s):
    ids, off, idx = csr(s["fv"])
    idx = idx if len(idx) else np.zeros(1, np.int32)
    keys, desc, hp = np.ascontiguousarray(s["keys"]), np.ascontiguousarray(s["desc"]), s.get("has_point")
    v = BowView(len(keys), keys.ctypes.data, desc.ctypes.data, hp.ctypes.data if hp is not None else None, None, len(ids), ids.ctypes.data,
                off.ctypes.data, idx.ctypes.data)
    return v, (keys, desc, hp, ids, off, idx)


def oracle_search(ob, kf, f, nn_ratio, check_orientation):
    """orc_search_by_bow -> (return value, matches_f)"""
    vk, keep_k = _view(kf)
    vf, keep_f = _view(f)
    m = np.zeros(max(vf.n, 1), np.int32)
    fn = ob.lib().orc_search_by_bow
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int]
    r = fn(C.byref(vk), C.byref(vf), m.ctypes.data_as(C.c_void_p), float(nn_ratio), int(check_orientation))
    return r, m[:vf.n].copy()


def flip(d, bits, rng):
    d = d.copy()
    for b in rng.choice(256, size=bits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def random_pair(seed, n_kf, n_f, n_nodes, has_point_share=None):
    """Clustered descriptors: every node has a centre; keyframe features lie near a centre, most frame features are a keyframe feature with a
    few bits flipped (so that they match and compete), in a node that is mostly, not always, the same."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 256, (n_nodes + 2, 32), dtype=np.uint8)
    node_kf = rng.integers(0, n_nodes + 1, n_kf)       # node n_nodes: on the keyframe's side only
    d_kf = np.array([flip(centres[c], int(rng.integers(0, 30)), rng) for c in node_kf])
    src = rng.integers(0, n_kf, n_f)
    d_f = np.array([flip(d_kf[s], int(rng.integers(0, 24)), rng) for s in src])
    node_f = np.where(rng.random(n_f) < 0.9, node_kf[src], rng.integers(0, n_nodes + 2, n_f))
    node_f[node_f == n_nodes] = n_nodes + 1            # node n_nodes + 1: on the frame's side only
    fv_kf, fv_f = {}, {}
    for i, c in enumerate(node_kf):
        fv_kf.setdefault(int(c) * 7 + 3, []).append(i)
    for i, c in enumerate(node_f):
        fv_f.setdefault(int(c) * 7 + 3, []).append(i)
    # angles on a grid of 12 degrees plus an offset: bins fill unevenly and some products land on .5
    ang_kf = (rng.integers(0, 30, n_kf) * 12.0 + rng.choice([0.0, 6.0, 3.3], n_kf)).astype(np.float32)
    ang_f = np.where(rng.random(n_f) < 0.7, ang_kf[src] - np.float32(24.0), rng.uniform(0, 360, n_f)).astype(np.float32) % np.float32(360.0)
    hp = None if has_point_share is None else (rng.random(n_kf) < has_point_share).astype(np.uint8)
    return side(d_kf, ang_kf, fv_kf, hp), side(d_f, ang_f, fv_f)


# ---------------------------------------------------------------------------------------------------------------- frames of the synth stream

SIZES = {"small": (320, 240, 500, 4), "large": (640, 480, 1000, 8)}  # width, height, features, levels
NODE_LEVELS = {"100": 1, "10": 2}  # the k = 10 / L = 3 vocabulary: levelsup 1 -> about 100 nodes, 2 -> about 10
_cache = {}


def vocabulary():
    import bow_restatement as br
    if "voc" not in _cache:
        _cache["voc"] = br.make_vocabulary(10, 3, seed=31, flips=100, bad_weight_share=0.05)
    return _cache["voc"]


def synth_sides(ob, synth, size, nodes):
    """Four frames of the synth stream at `size`, extracted by the CPU oracle, with the FeatureVector the restatement gives each at the
    levelsup of `nodes`; has_point marks 80 % of the features.  Computed once per (size, nodes)."""
    import bow_restatement as br
    key = (size, nodes)
    if key not in _cache:
        w, h, nf, nl = SIZES[size]
        if ("frames", size) not in _cache:
            orc = ob.Oracle(nf, 1.2, nl)
            _cache[("frames", size)] = [orc.extract(synth.frame(3, k, h, w)) for k in range(4)]
        rng = np.random.default_rng(w + len(nodes))
        out = []
        for kps, desc in _cache[("frames", size)]:
            fv = br.transform(vocabulary(), desc, NODE_LEVELS[nodes])["fv"]
            s = side(desc, kps["angle"], fv, (rng.random(len(kps)) < 0.8).astype(np.uint8))
            s["keys"] = np.ascontiguousarray(kps, KP)
            out.append(s)
        _cache[key] = out
    return _cache[key]


PAIRS = [(0, 1), (2, 1), (3, 1), (1, 0)]  # (keyframe, frame): three keyframes against one frame is the relocalisation shape


# ---------------------------------------------------------------------------------------------------------------- hand cases

def _d(*bits):
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def _first(n):
    return _d(*range(n))


def hand_cases():
    """name -> (kf, f, nn_ratio, check_orientation, expected matches_f, expected n_matches)"""
    zero, ones = _first(0), _first(256)
    c = {}
    # three keyframe features compete for frame feature 0 (distances 3, 1, 2 in turn; feature 1 is far): the first takes it, the others
    # see only the far one
    c["three_compete"] = (side([_first(3), _first(1), _first(2)], [0, 0, 0], {5: [0, 1, 2]}), side([zero, _first(120)], [0, 0], {5: [0, 1]}),
                          0.7, 0, [0, -1], 1)
    # a lone candidate: the second best stays 256
    c["lone_candidate"] = (side([_first(20)], [0], {5: [0]}), side([zero], [0], {5: [0]}), 0.7, 0, [0], 1)
    # a complement is at distance 256: never a candidate, so the other one is a lone candidate at distance 40
    c["complement"] = (side([zero], [0], {5: [0]}), side([ones, _first(40)], [0, 0], {5: [0, 1]}), 0.7, 0, [-1, 0], 1)
    c["only_a_complement"] = (side([zero], [0], {5: [0]}), side([ones], [0], {5: [0]}), 0.7, 0, [-1], 0)
    # distance exactly 50 is accepted, 51 is not
    c["distance_50"] = (side([zero], [0], {5: [0]}), side([_first(50)], [0], {5: [0]}), 0.7, 0, [0], 1)
    c["distance_51"] = (side([zero], [0], {5: [0]}), side([_first(51)], [0], {5: [0]}), 0.7, 0, [-1], 0)
    # an exact ratio tie: 0.75f * 40 == 30 is not < under the strict comparison; 29 is
    c["ratio_tie"] = (side([zero], [0], {5: [0]}), side([_first(30), _first(40)], [0, 0], {5: [0, 1]}), 0.75, 0, [-1, -1], 0)
    c["ratio_below_tie"] = (side([zero], [0], {5: [0]}), side([_first(29), _first(40)], [0, 0], {5: [0, 1]}), 0.75, 0, [0, -1], 1)
    # equal distances: the first of the list wins, and the ratio test fails on the tie (10 < 0.7 * 10 is false)
    c["equal_distances"] = (side([zero], [0], {5: [0]}), side([_d(1, 2), _d(3, 4)], [0, 0], {5: [1, 0]}), 0.7, 0, [-1, -1], 0)
    # nodes on one side only take no part
    c["one_sided_nodes"] = (side([zero, zero], [0, 0], {3: [0], 9: [1]}), side([zero, zero], [0, 0], {4: [0], 9: [1]}), 0.7, 0, [-1, 1], 1)
    c["empty_vectors"] = (side([zero, zero], [0, 0], {}), side([zero], [0], {}), 0.7, 1, [-1], 0)
    c["no_features"] = (side(np.zeros((0, 32), np.uint8), [], {}), side(np.zeros((0, 32), np.uint8), [], {}), 0.7, 1, [], 0)
    c["no_map_points"] = (side([zero], [0], {5: [0]}, [0]), side([zero], [0], {5: [0]}), 0.7, 0, [-1], 0)
    # a histogram tie among the maxima: bins 0, 5, 10 and 15 hold 2, 2, 2, 2 matches: the three EARLIEST bins stay (strict comparisons)
    n = 8
    descs = [_d(*range(16 * i, 16 * i + 8)) for i in range(n)]  # 16 bits apart from each other
    ang_kf = [0, 0, 60, 60, 120, 120, 180, 180]
    c["histogram_tie"] = (side(descs, ang_kf, {5: list(range(n))}), side(descs, [0] * n, {5: list(range(n))}), 0.7, 1,
                          [0, 1, 2, 3, 4, 5, -1, -1], 6)
    # a bin of 30 becomes 0: rot = 354.1 -> 29.508 -> 30 -> 0; with rot 0 also in bin 0 and one match in bin 15, max2 = 1 >= 0.1 * 2 stays
    c["bin_30_wraps"] = (side(descs[:3], [354.1, 0, 180], {5: [0, 1, 2]}), side(descs[:3], [0, 0, 0], {5: [0, 1, 2]}), 0.7, 1, [0, 1, 2], 3)
    return c
