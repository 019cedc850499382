"""Inputs of the keyframe pair search tests (SearchForTriangulation, SearchByBoW(KF, KF)) and orc_search_for_triangulation /
orc_search_by_bow_kf (oracle/orb_oracle.c) bound for them.  A side is the dict of bow_search_cases.py plus u_right (float32 [n], or None:
monocular); for SearchByBoW(KF, KF) has_point marks the good map points, for triangulation it marks the features that HAVE a point."""
import numpy as np

import bow_search_cases as bc

f32 = np.float32
KP = bc.KP
STAT_FIELDS = ("n_queries", "n_matches", "n_researched")


def side(desc, angles, fv, has_point=None, xy=None, octave=None, u_right=None):
    s = bc.side(desc, angles, fv, has_point)
    n = len(s["desc"])
    if xy is not None:
        xy = np.asarray(xy, f32).reshape(n, 2)
        s["keys"]["x"], s["keys"]["y"] = xy[:, 0], xy[:, 1]
    if octave is not None:
        s["keys"]["octave"] = np.asarray(octave, np.int32)
    s["u_right"] = None if u_right is None else np.ascontiguousarray(u_right, f32)
    return s


with_csr = bc.with_csr


def _view(s):
    import host_binding as hb
    return hb.bow_view(s["keys"], s["desc"], s["fv"], s.get("has_point"), s.get("u_right"))


def oracle_bow_kf(k1, k2, nn_ratio, check_orientation):
    """orc_search_by_bow_kf -> (return value, match12)"""
    import host_binding as hb
    v1, keep1 = _view(k1)
    v2, keep2 = _view(k2)
    r, m = hb.search_bow_kf("oracle", v1, v2, nn_ratio, int(check_orientation))
    return r, m.copy()


def oracle_triangulation(k1, k2, geo, scale_factors, level_sigma2, only_stereo, check_orientation):
    """orc_search_for_triangulation -> (return value, match12 rebuilt from its pairs, which ascend in idx1)"""
    import host_binding as hb
    v1, keep1 = _view(k1)
    v2, keep2 = _view(k2)
    r, pairs = hb.search_triangulation("oracle", v1, v2, geo["f12"], float(geo["ex"]), float(geo["ey"]), scale_factors, level_sigma2,
                                       int(only_stereo), int(check_orientation))
    m = np.full(v1.n, -1, np.int32)
    assert (np.diff(pairs[:, 0]) > 0).all()
    m[pairs[:, 0]] = pairs[:, 1]
    return r, m


# ---------------------------------------------------------------------------------------------------------------- geometry

GEOMETRY = np.dtype([("f12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4")])  # amos_kf_geometry


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def geometry(K, R12, t12):
    """F12 = K^-T [t12]x R12 K^-1 (LocalMapping::ComputeF12) in float64, cast to float32, and keyframe 1's centre in keyframe 2's image as
    ORBmatcher.cc:818-825 computes it in float32 (an epipole at infinity stays infinite / not a number: its test then rejects nothing)."""
    K, R12, t12 = np.asarray(K, np.float64), np.asarray(R12, np.float64), np.asarray(t12, np.float64)
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R12 @ Ki
    F = F / np.abs(F).max()
    C2 = (-R12.T @ t12).astype(f32)
    g = np.zeros((), GEOMETRY)
    g["f12"] = F.astype(f32).reshape(9)
    with np.errstate(all="ignore"):
        invz = f32(1.0) / C2[2]
        g["ex"] = f32(K[0, 0]) * C2[0] * invz + f32(K[0, 2])
        g["ey"] = f32(K[1, 1]) * C2[1] * invz + f32(K[1, 2])
    return g


def camera(w, h):
    return np.array([[0.84 * w, 0, 0.5 * w + 0.3], [0, 0.85 * w, 0.5 * h - 0.4], [0, 0, 1]], np.float64)


def shift_motions(w, h):
    """name -> (R12, t12) for two keyframes whose features differ by an image shift along (2, 1) (the synth stream): a pure x-translation
    (horizontal lines: the shift's y part is the distance to the line), a pure y-translation (vertical lines: its x part), and a small
    rotation plus a translation along the shift with some forward motion (the epipole lies far outside the image)."""
    K = camera(w, h)
    along = np.array([2.0 / K[0, 0], 1.0 / K[1, 1], 0.0])
    return {"x": (np.eye(3), np.array([1.0, 0.0, 0.0])), "y": (np.eye(3), np.array([0.0, 1.0, 0.0])),
            "general": (_rot(2e-4, -3e-4, 5e-4), along + [0.0, 0.0, 1.5e-4])}


def shift_geometries(w, h):
    return {k: geometry(camera(w, h), R, t) for k, (R, t) in shift_motions(w, h).items()}


def levels(n_levels, factor=1.2):
    sf = np.cumprod([1.0] + [factor] * (n_levels - 1)).astype(f32)
    return sf, (sf * sf).astype(f32)


# ---------------------------------------------------------------------------------------------------------------- random pairs

def random_pair(seed, n1=70, n2=80, n_nodes=4, point_share=0.3, stereo_share=0.4, geometry_kind="forward"):
    """bow_search_cases.random_pair's clustered descriptors as two keyframes with positions that obey ONE geometry: keyframe 1's features
    are back-projected at random depths and projected into keyframe 2 (a keyframe-2 feature takes its source's projection plus up to two
    pixels of noise, or a random place); "forward" moves the camera mostly along its axis, so the epipole lies inside the image and mono
    features fall within its radius."""
    k1, k2 = bc.random_pair(seed, n1, n2, n_nodes)
    rng = np.random.default_rng(seed + 1000)
    w, h, nl = 640, 480, 8
    K = camera(w, h)
    R12, t12 = (_rot(1e-3, -2e-3, 1.5e-3), np.array([0.02, -0.01, 0.3])) if geometry_kind == "forward" else (np.eye(3), np.array([0.2, 0.0, 0.0]))
    # keyframe 2's descriptors were drawn from keyframe 1's: recover the source as the nearest keyframe-1 descriptor
    import bow_restatement as br
    src = br._POP[np.bitwise_xor(k2["desc"][:, None, :], k1["desc"][None, :, :])].sum(2).argmin(1)
    xy1 = np.stack([rng.uniform(20, w - 20, n1), rng.uniform(20, h - 20, n1)], 1)
    if geometry_kind == "forward":  # a share near the epipole
        C2 = -R12.T @ t12
        xy1[: n1 // 3] = K[:2, 2] + K[[0, 1], [0, 1]] * C2[:2] / C2[2] + rng.uniform(-14, 14, (n1 // 3, 2))
    depth = rng.uniform(1.0, 8.0, n1)
    X1 = (np.linalg.inv(K) @ np.concatenate([xy1, np.ones((n1, 1))], 1).T) * depth  # 3 x n1, in keyframe 1's frame
    X2 = R12.T @ (X1 - t12[:, None])                                                 # X1 = R12 X2 + t12
    p2 = (K @ X2)[:2] / X2[2]
    xy2 = p2.T[src] + rng.uniform(-2.0, 2.0, (n2, 2)) * (rng.random((n2, 1)) < 0.5)
    stray = rng.random(n2) < 0.15
    xy2[stray] = np.stack([rng.uniform(0, w, stray.sum()), rng.uniform(0, h, stray.sum())], 1)
    o1, o2 = rng.integers(0, nl, n1), rng.integers(0, nl, n2)
    ur1 = np.where(rng.random(n1) < stereo_share, xy1[:, 0] - rng.uniform(3, 30, n1), -1.0)
    ur2 = np.where(rng.random(n2) < stereo_share, xy2[:, 0] - rng.uniform(3, 30, n2), -1.0)
    hp1, hp2 = (rng.random(n1) < point_share).astype(np.uint8), (rng.random(n2) < point_share).astype(np.uint8)
    s1 = side(k1["desc"], k1["angles"], k1["fv"], hp1, xy1, o1, ur1)
    s2 = side(k2["desc"], k2["angles"], k2["fv"], hp2, xy2, o2, ur2)
    return s1, s2, geometry(K, R12, t12), levels(nl)


# ---------------------------------------------------------------------------------------------------------------- frames of the synth stream

PAIRS = [(1, 0), (1, 2), (1, 3), (0, 1)]            # (keyframe 1, keyframe 2): three against one keyframe 1 (the LocalMapping shape), one reversed
PAIR_GEOMETRY = ["x", "y", "general", "general"]    # frame k is the scene moved by (2 k, k) pixels
_cache = {}


def synth_sides(ob, synth, size, nodes, point_share):
    """bow_search_cases.synth_sides with has_point redrawn at `point_share` and about 40 % of the features stereo"""
    key = (size, nodes, point_share)
    if key not in _cache:
        rng = np.random.default_rng(int(point_share * 100) + len(nodes))
        out = []
        for s in bc.synth_sides(ob, synth, size, nodes):
            n = len(s["desc"])
            s = dict(s, has_point=(rng.random(n) < point_share).astype(np.uint8))
            s["u_right"] = np.where(rng.random(n) < 0.4, s["keys"]["x"] - rng.uniform(3, 30, n), -1.0).astype(f32)
            out.append(s)
        _cache[key] = out
    return _cache[key]


def synth_geometry(size):
    w, h, _, nl = bc.SIZES[size]
    return shift_geometries(w, h), levels(nl)


# ---------------------------------------------------------------------------------------------------------------- the resident arrays

def pack(sides, cap, hp_none=0):
    """the resident arrays of the frame slots, with padding that must not be read as data; a side without has_point gets hp_none (what a
    NULL has_point means to the search: 0 for triangulation, 1 for SearchByBoW), one without u_right -1"""
    ns = len(sides)
    a = dict(kps=np.zeros((ns, cap), KP), desc=np.full((ns, cap, 32), 0x3C, np.uint8), counts=np.zeros(ns, np.int32),
             n_nodes=np.zeros(ns, np.int32), node_ids=np.full((ns, cap), 0xABABABAB, np.uint32), node_off=np.full((ns, cap + 1), -77, np.int32),
             node_idx=np.full((ns, cap), -55, np.int32), has_point=np.full((ns, cap), 7, np.uint8), u_right=np.full((ns, cap), 3.0, f32))
    for s, sd in enumerate(sides):
        n = len(sd["desc"])
        ids, off, idx = bc.csr(sd["fv"])
        a["counts"][s], a["n_nodes"][s] = n, len(ids)
        a["kps"][s, :n], a["desc"][s, :n] = sd["keys"], sd["desc"]
        a["node_ids"][s, :len(ids)], a["node_off"][s, :len(off)], a["node_idx"][s, :len(idx)] = ids, off, idx
        a["has_point"][s, :n] = sd["has_point"] if sd.get("has_point") is not None else hp_none
        a["u_right"][s, :n] = sd["u_right"] if sd.get("u_right") is not None else -1.0
    return a


# ---------------------------------------------------------------------------------------------------------------- hand cases

_d, _first = bc._d, bc._first
K_HAND = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]])
G_X = geometry(K_HAND, np.eye(3), [1.0, 0.0, 0.0])          # horizontal lines: dsqr = (y2 - y1)^2
G_FORWARD = geometry(K_HAND, np.eye(3), [0.0, 0.0, 1.0])    # the epipole is the principal point (320, 240): lines through it
G_ZERO = np.zeros((), GEOMETRY)                             # F12 = 0: den == 0 for every feature


def bow_kf_hand_cases():
    """name -> (k1, k2, nn_ratio, check_orientation, expected match12, expected n_matches)"""
    zero = _first(0)
    c = {}
    c["first_of_equal_wins"] = (side([zero], [0], {5: [0]}), side([_d(1, 2), _d(3, 4)], [0, 0], {5: [1, 0]}), 1.5, 0, [1], 1)
    c["distance_49"] = (side([zero], [0], {5: [0]}), side([_first(49)], [0], {5: [0]}), 0.75, 0, [0], 1)
    c["distance_50"] = (side([zero], [0], {5: [0]}), side([_first(50)], [0], {5: [0]}), 0.75, 0, [-1], 0)
    c["ratio_tie"] = (side([zero], [0], {5: [0]}), side([_first(30), _first(40)], [0, 0], {5: [0, 1]}), 0.75, 0, [-1], 0)
    c["ratio_below_tie"] = (side([zero], [0], {5: [0]}), side([_first(29), _first(40)], [0, 0], {5: [0, 1]}), 0.75, 0, [0], 1)
    # keyframe 2's nearest feature has no good map point: it is no candidate, the far one is a lone candidate
    c["candidate_without_point"] = (side([zero], [0], {5: [0]}), side([_first(2), _first(30)], [0, 0], {5: [0, 1]}, [0, 1]), 0.75, 0, [1], 1)
    c["query_without_point"] = (side([zero, zero], [0, 0], {5: [0, 1]}, [0, 1]), side([zero], [0], {5: [0]}), 0.75, 0, [-1, 0], 1)
    # three compete for keyframe-2 feature 0: the first takes it; the second then sees 1 (dist 21) and 2 (far): accepted; the third sees only 2
    c["three_compete"] = (side([_first(3), _first(1), _first(2)], [0, 0, 0], {5: [0, 1, 2]}),
                          side([zero, _d(*range(100, 120)), _d(*range(130, 250))], [0, 0, 0], {5: [0, 1, 2]}), 0.75, 0, [0, 1, -1], 2)
    c["one_sided_nodes"] = (side([zero, zero], [0, 0], {3: [0], 9: [1]}), side([zero, zero], [0, 0], {4: [0], 9: [1]}), 0.75, 0, [-1, 1], 1)
    c["empty_vectors"] = (side([zero, zero], [0, 0], {}), side([zero], [0], {}), 0.75, 1, [-1, -1], 0)
    c["no_features"] = (side(np.zeros((0, 32), np.uint8), [], {}), side(np.zeros((0, 32), np.uint8), [], {}), 0.75, 1, [], 0)
    n = 8
    descs = [_d(*range(16 * i, 16 * i + 8)) for i in range(n)]  # 16 bits apart from each other
    c["histogram_tie"] = (side(descs, [0, 0, 60, 60, 120, 120, 180, 180], {5: list(range(n))}), side(descs, [0] * n, {5: list(range(n))}), 0.75, 1,
                          [0, 1, 2, 3, 4, 5, -1, -1], 6)
    c["bin_30_wraps"] = (side(descs[:3], [354.1, 0, 180], {5: [0, 1, 2]}), side(descs[:3], [0, 0, 0], {5: [0, 1, 2]}), 0.75, 1, [0, 1, 2], 3)
    return c


def triangulation_hand_cases():
    """name -> (k1, k2, geometry, only_stereo, check_orientation, expected match12, expected n_matches); 8 levels of factor 1.2"""
    zero = _first(0)
    c = {}

    def one(d2, xy2, **kw):  # one mono feature at (100, 100) against keyframe 2
        return side([zero], [0], {5: [0]}, xy=[[100, 100]]), side(d2, [0] * len(d2), {5: list(range(len(d2)))}, xy=xy2, **kw)
    # equal distances, both on the line: the LAST of the list wins
    c["last_of_equal_wins"] = (*one([_d(1, 2), _d(3, 4), _d(5, 6)], [[90, 100], [80, 100], [70, 100]]), G_X, 0, 0, [2], 1)
    # the last of equal distances is off the line: the one before it stays
    c["last_of_equal_off_line"] = (*one([_d(1, 2), _d(3, 4), _d(5, 6)], [[90, 100], [80, 100], [70, 150]]), G_X, 0, 0, [1], 1)
    c["distance_50"] = (*one([_first(50)], [[90, 100]]), G_X, 0, 0, [0], 1)
    c["distance_51"] = (*one([_first(51)], [[90, 100]]), G_X, 0, 0, [-1], 0)
    c["den_zero"] = (*one([zero], [[90, 100]]), G_ZERO, 0, 0, [-1], 0)
    # dsqr = 1.9^2 = 3.61 < 3.84 at octave 0, 2.0^2 = 4 is not; at octave 1 (sigma2 1.44) 4 < 5.53
    c["line_inside"] = (*one([zero], [[90, 101.9]]), G_X, 0, 0, [0], 1)
    c["line_outside"] = (*one([zero], [[90, 102.0]]), G_X, 0, 0, [-1], 0)
    c["line_octave_1"] = (*one([zero], [[90, 102.0]], octave=[1]), G_X, 0, 0, [0], 1)
    # the epipole radius: 100 * 1.0 at octave 0; (320 - 310)^2 = 100 is not below it (kept), 99.8 is (rejected); the feature of keyframe 1
    # lies on the same line through the epipole
    k1e = side([zero], [0], {5: [0]}, xy=[[200, 240]])
    c["at_epipole_radius"] = (k1e, side([zero], [0], {5: [0]}, xy=[[310, 240]]), G_FORWARD, 0, 0, [0], 1)
    c["inside_epipole_radius"] = (k1e, side([zero], [0], {5: [0]}, xy=[[310.01, 240]]), G_FORWARD, 0, 0, [-1], 0)
    # ... a stereo feature on either side skips the epipole test
    c["inside_epipole_radius_stereo"] = (k1e, side([zero], [0], {5: [0]}, xy=[[310.01, 240]], u_right=[300.0]), G_FORWARD, 0, 0, [0], 1)
    # stereo / mono mix: keyframe 1 (mono, stereo), keyframe 2 (stereo nearest to both, mono)
    mix1 = side([zero, _first(1)], [0, 0], {5: [0, 1]}, xy=[[100, 100], [100, 120]], u_right=[-1, 90])
    mix2 = side([_first(2), _first(9), _first(12)], [0, 0, 0], {5: [0, 1, 2]}, xy=[[90, 100], [80, 120], [70, 100]], u_right=[80, -1, -1])
    c["mix_all"] = (mix1, mix2, G_X, 0, 0, [0, 1], 2)
    c["mix_only_stereo"] = (mix1, mix2, G_X, 1, 0, [-1, -1], 0)
    mix3 = side([_first(2), _first(9)], [0, 0], {5: [0, 1]}, xy=[[90, 120], [80, 120]], u_right=[-1, 60])
    c["mix_only_stereo_match"] = (mix1, mix3, G_X, 1, 0, [-1, 1], 1)
    c["mono_views_under_only_stereo"] = (*one([zero], [[90, 100]]), G_X, 1, 0, [-1], 0)
    # features with a map point: skipped on side 1, no candidate on side 2
    c["map_points"] = (side([zero, zero], [0, 0], {5: [0, 1]}, [1, 0], xy=[[100, 100], [100, 100]]),
                       side([zero, _first(3)], [0, 0], {5: [0, 1]}, [1, 0], xy=[[90, 100], [80, 100]]), G_X, 0, 0, [-1, 1], 1)
    # best taken, second free: three queries on one row; candidates at distances (q0: 0, 20; q1: 1, 19 -> takes the second)
    row = dict(xy=[[100, 100]] * 3)
    c["best_taken_second_free"] = (side([zero, _first(1)], [0, 0], {5: [0, 1]}, xy=[[100, 100]] * 2),
                                   side([zero, _first(20)], [0, 0], {5: [0, 1]}, xy=[[90, 100], [80, 100]]), G_X, 0, 0, [0, 1], 2)
    c["best_taken_no_second"] = (side([zero, _first(1)], [0, 0], {5: [0, 1]}, xy=[[100, 100]] * 2),
                                 side([zero], [0], {5: [0]}, xy=[[90, 100]]), G_X, 0, 0, [0, -1], 1)
    # both taken: q0 takes feature 0, q1 takes feature 1 (its best, 0, is taken), q2's best two (0, 1) are taken: the new search finds 2
    c["both_taken"] = (side([zero, _first(1), _first(2)], [0, 0, 0], {5: [0, 1, 2]}, **row),
                       side([zero, _first(10), _first(30)], [0, 0, 0], {5: [0, 1, 2]}, xy=[[90, 100], [80, 100], [70, 100]]), G_X, 0, 0, [0, 1, 2], 3)
    c["both_taken_nothing_left"] = (side([zero, _first(1), _first(2)], [0, 0, 0], {5: [0, 1, 2]}, **row),
                                    side([zero, _first(10)], [0, 0], {5: [0, 1]}, xy=[[90, 100], [80, 100]]), G_X, 0, 0, [0, 1, -1], 2)
    c["one_sided_nodes"] = (side([zero, zero], [0, 0], {3: [0], 9: [1]}, xy=[[100, 100]] * 2),
                            side([zero, zero], [0, 0], {4: [0], 9: [1]}, xy=[[90, 100]] * 2), G_X, 0, 0, [-1, 1], 1)
    c["empty_vectors"] = (side([zero, zero], [0, 0], {}), side([zero], [0], {}), G_X, 0, 1, [-1, -1], 0)
    c["no_features"] = (side(np.zeros((0, 32), np.uint8), [], {}), side(np.zeros((0, 32), np.uint8), [], {}), G_X, 0, 1, [], 0)
    n = 8
    descs = [_d(*range(16 * i, 16 * i + 8)) for i in range(n)]
    xy = [[100 + 10 * i, 50 + 20 * i] for i in range(n)]
    c["histogram_tie"] = (side(descs, [0, 0, 60, 60, 120, 120, 180, 180], {5: list(range(n))}, xy=xy),
                          side(descs, [0] * n, {5: list(range(n))}, xy=xy), G_X, 0, 1, [0, 1, 2, 3, 4, 5, -1, -1], 6)
    c["bin_30_wraps"] = (side(descs[:3], [354.1, 0, 180], {5: [0, 1, 2]}, xy=xy[:3]), side(descs[:3], [0, 0, 0], {5: [0, 1, 2]}, xy=xy[:3]),
                         G_X, 0, 1, [0, 1, 2], 3)
    return c


HAND_LEVELS = levels(8)
