"""Inputs of the new-map-point tests (amos_match_new_points_batch_device, its host form and drop-in): hand cases, one per verdict and per
quirk of LocalMapping.cc:424-597 that the core header keeps, the random pairs of kf_search_cases.py extended with the two poses behind
their R12 / t12 and depths consistent with u_right, and the synth keyframes at 160 x 120.  A case is a dict: sides (one per frame slot:
keys, u_right, depth, keys_raw; the random and synth ones also carry what the search reads), cams (KF_CAMERA records), pairs, match (one
row per pair), enabled (or None), levels.  check_cases() asserts, in the restatement, that the cases do what they are named for."""
import numpy as np

import bow_search_cases as bc
import kf_search_cases as kc
import new_points_restatement as nr

f32 = np.float32
KP = bc.KP
K_HAND = (500.0, 500.0, 320.0, 240.0)
MB, MBF = 0.08, 40.0
HAND_LEVELS = kc.HAND_LEVELS
CAPACITY = 8


def _roty(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def hand_cam(centre=(0.0, 0.0, 0.0), R=None, mbf=MBF, mb=MB):
    """a camera at `centre` (world coordinates) with world -> camera rotation R"""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    return nr.camera(R, -R @ np.asarray(centre, np.float64), K_HAND, mb, mbf, 1.2)


def project(cam, P):
    """the pixel and the depth of world point P in float64"""
    R, t = cam["Rcw"].astype(np.float64).reshape(3, 3), cam["tcw"].astype(np.float64)
    X = R @ np.asarray(P, np.float64) + t
    return float(cam["fx"]) * X[0] / X[2] + float(cam["cx"]), float(cam["fy"]) * X[1] / X[2] + float(cam["cy"]), X[2]


def mk_side(xy, octave=None, u_right=None, depth=None, raw_xy=None):
    n = len(xy)
    keys = np.zeros(n, KP)
    xy = np.asarray(xy, f32).reshape(n, 2)
    keys["x"], keys["y"] = xy[:, 0], xy[:, 1]
    if octave is not None:
        keys["octave"] = np.asarray(octave, np.int32)
    s = {"keys": keys, "u_right": None if u_right is None else np.asarray(u_right, f32), "depth": None if depth is None else np.asarray(depth, f32),
         "keys_raw": None}
    if raw_xy is not None:
        raw = keys.copy()
        raw_xy = np.asarray(raw_xy, f32).reshape(n, 2)
        raw["x"], raw["y"] = raw_xy[:, 0], raw_xy[:, 1]
        s["keys_raw"] = raw
    return s


def _case(sides, cams, pairs, match, expect, enabled=None, status=None):
    return {"sides": sides, "cams": cams, "pairs": pairs, "match": [np.asarray(m, np.int32) for m in match], "enabled": enabled,
            "levels": HAND_LEVELS, "expect": expect, "status": status or [0] * len(pairs)}


P0 = (0.5, 0.2, 4.0)


def _two(P, c1, c2, d1=(0.0, 0.0), d2=(0.0, 0.0), o1=0, o2=0, stereo1=None, stereo2=None, raw1=None):
    """one feature per keyframe: P's projections moved by d1 / d2 pixels.  stereoN = (u_right offset from the consistent value, depth) or
    None for a mono feature; raw1: the raw keypoint's offset from the undistorted one"""
    sides = []
    for cam, d, o, st, raw in ((c1, d1, o1, stereo1, raw1), (c2, d2, o2, stereo2, None)):
        u, v, z = project(cam, P)
        xy = [[u + d[0], v + d[1]]]
        ur = dp = None
        if st is not None:
            ur, dp = [u - MBF / z + st[0]], [st[1]]
        sides.append(mk_side(xy, [o], ur, dp, None if raw is None else [[xy[0][0] + raw[0], xy[0][1] + raw[1]]]))
    return sides


def hand_cases():
    """name -> case; `expect`: per pair the verdict of every keyframe-1 feature"""
    c = {}
    near, wide = hand_cam((0.01, 0, 0)), hand_cam((0.5, 0, 0))
    c0 = hand_cam()
    c["triangulated"] = _case(_two(P0, c0, wide), [c0, wide], [(0, 1)], [[0]], [[nr.TRIANGULATED]])
    c["unprojected_1"] = _case(_two(P0, c0, near, stereo1=(0, 4.0)), [c0, near], [(0, 1)], [[0]], [[nr.UNPROJECTED_1]])
    c["unprojected_2"] = _case(_two(P0, c0, near, stereo2=(0, 4.0)), [c0, near], [(0, 1)], [[0]], [[nr.UNPROJECTED_2]])
    c["low_parallax_small_angle"] = _case(_two(P0, c0, near), [c0, near], [(0, 1)], [[0]], [[nr.LOW_PARALLAX]])
    turned = hand_cam((0.5, 0, 0), _roty(np.radians(120)))
    c["low_parallax_cos_negative"] = _case([mk_side([[320, 240]]), mk_side([[320, 240]])], [c0, turned], [(0, 1)], [[0]], [[nr.LOW_PARALLAX]])
    # both stereo: only cosParallaxStereo1 is computed (a depth of 400: about 1), so the rays' cosine is below the bound and the match is
    # triangulated; with cosParallaxStereo2 (depth 4: 0.9998) it would have been UnprojectStereo of keyframe 2
    c["both_stereo_else_if"] = _case(_two(P0, c0, near, stereo1=(0, 400.0), stereo2=(0, 4.0)), [c0, near], [(0, 1)], [[0]], [[nr.TRIANGULATED]])
    # the rays through these two pixels meet at (0.25, 0, -4): behind both cameras
    back = (0.25, 0.0, -4.0)
    c["behind_1"] = _case(_two(back, c0, wide), [c0, wide], [(0, 1)], [[0]], [[nr.BEHIND_1]])
    ahead = hand_cam((0, 0, 8.0))  # keyframe 2 stands beyond the point that keyframe 1 unprojects
    c["behind_2"] = _case([_two(P0, c0, c0, stereo1=(0, 4.0))[0], mk_side([[382.5, 265.0]])], [c0, ahead], [(0, 1)], [[0]], [[nr.BEHIND_2]])
    c["reprojection_1_mono"] = _case(_two(P0, c0, wide, d1=(0, 10)), [c0, wide], [(0, 1)], [[0]], [[nr.REPROJECTION_1]])
    c["reprojection_1_stereo"] = _case(_two(P0, c0, wide, stereo1=(5, 4.0)), [c0, wide], [(0, 1)], [[0]], [[nr.REPROJECTION_1]])
    c["reprojection_2_mono"] = _case(_two(P0, c0, near, d2=(5, 0), stereo1=(0, 4.0)), [c0, near], [(0, 1)], [[0]], [[nr.REPROJECTION_2]])
    c["reprojection_2_stereo"] = _case(_two(P0, c0, near, stereo1=(0, 4.0), stereo2=(5, 4.0)), [c0, near], [(0, 1)], [[0]], [[nr.REPROJECTION_2]])
    # keyframe 2's u_right fits ITS mbf (20: a disparity of 5); the reference projects with keyframe 1's (40: 10) and rejects
    near20 = hand_cam((0.01, 0, 0), mbf=20.0)
    s = _two(P0, c0, near20, stereo1=(0, 4.0), stereo2=(0, 4.0))
    s[1]["u_right"] = (s[1]["keys"]["x"] - f32(20.0 / 4.0)).astype(f32)
    c["reprojection_2_other_mbf"] = _case(s, [c0, near20], [(0, 1)], [[0]], [[nr.REPROJECTION_2]])
    c["unprojected_1_raw_keys"] = _case(_two(P0, c0, near, stereo1=(0, 4.0), raw1=(1.5, -1.0)), [c0, near], [(0, 1)], [[0]], [[nr.UNPROJECTED_1]])
    c["scale_below"] = _case(_two(P0, c0, wide, o1=4, o2=0), [c0, wide], [(0, 1)], [[0]], [[nr.SCALE]])
    c["scale_above"] = _case(_two(P0, c0, wide, o1=0, o2=4), [c0, wide], [(0, 1)], [[0]], [[nr.SCALE]])
    c["octave_1"] = _case(_two(P0, c0, wide, o1=8), [c0, wide], [(0, 1)], [[0]], [[nr.OCTAVE]], status=[nr.BAD_OCTAVE])
    c["octave_2"] = _case(_two(P0, c0, wide, o2=-1), [c0, wide], [(0, 1)], [[0]], [[nr.OCTAVE]], status=[nr.BAD_OCTAVE])
    # two features in keyframe 1, one in keyframe 2: entries 1 and -7 name no keyframe-2 feature
    s = _two(P0, c0, wide)
    s[0] = mk_side([list(project(c0, P0)[:2]), [100.0, 100.0]])
    c["match_out_of_range"] = _case(s, [c0, wide], [(0, 1)], [[1, -7]], [[-1, -1]], status=[nr.BAD_MATCH])
    # three neighbours of one keyframe 1, two features.  Feature 0: accepted in pairs 0 and 2 (CLAIMED there), rejected in pair 1.
    # Feature 1: rejected in pair 0, accepted in pair 1, accepted in pair 2 (CLAIMED)
    P1 = (-0.4, 0.3, 5.0)
    n1, n2, n3 = hand_cam((0.5, 0, 0)), hand_cam((0, 0.5, 0)), hand_cam((-0.5, 0, 0))

    def pix(cam, P, d=(0.0, 0.0)):
        u, v, _ = project(cam, P)
        return [u + d[0], v + d[1]]
    sides = [mk_side([pix(c0, P0), pix(c0, P1)]), mk_side([pix(n1, P0), pix(n1, P1, (0, 12))]), mk_side([pix(n2, P0, (12, 0)), pix(n2, P1)]),
             mk_side([pix(n3, P0), pix(n3, P1)])]
    c["claimed"] = _case(sides, [c0, n1, n2, n3], [(0, 1), (0, 2), (0, 3)], [[0, 1]] * 3,
                         [[nr.TRIANGULATED, nr.REPROJECTION_1], [nr.REPROJECTION_1, nr.TRIANGULATED], [nr.CLAIMED, nr.CLAIMED]])
    return c


def run_case(case):
    return nr.new_points(case["sides"], case["cams"], case["pairs"], case["match"], case["levels"], case["enabled"])


# ---------------------------------------------------------------------------------------------------------------- random pairs

MOTIONS = {"forward": (kc._rot(1e-3, -2e-3, 1.5e-3), np.array([0.02, -0.01, 0.3])), "sideways": (np.eye(3), np.array([0.2, 0.0, 0.0]))}  # kc.random_pair's
RANDOM_SEEDS = (5, 6)
RANDOM_KINDS = ("forward", "sideways")
_cache = {}


def pose_cameras(K, R12, t12, mb, scale_factor=1.2):
    """keyframe 1 is the world frame; X1 = R12 X2 + t12, so keyframe 2's pose is R12^T | -R12^T t12"""
    Kt = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    mbf = mb * K[0, 0]
    return [nr.camera(np.eye(3), np.zeros(3), Kt, mb, mbf, scale_factor), nr.camera(R12.T, -R12.T @ t12, Kt, mb, mbf, scale_factor)]


def with_depth(s, mbf):
    """depths consistent with u_right: mbf / disparity in float32 (mono features: -1)"""
    ur = s["u_right"]
    with np.errstate(all="ignore"):
        depth = np.where(ur >= 0, f32(mbf) / (s["keys"]["x"] - ur), f32(-1.0)).astype(f32)
    return dict(s, depth=depth, keys_raw=None)


def random_case(seed, kind):
    """kc.random_pair(seed, 70, 80) as a case of two pairs on one keyframe 1: against keyframe 2 and against a second neighbour at the same
    pose whose features are keyframe 2's moved by up to 0.4 pixels (what pair 0 accepts is CLAIMED there).  A few keyframe-1 octaves lie
    outside the levels (the search does not read them); the raw keypoints of keyframe 1 differ from the undistorted ones.  match: the CPU
    oracle's search."""
    key = (seed, kind)
    if key not in _cache:
        k1, k2, geo, lv = kc.random_pair(seed, 70, 80, geometry_kind=kind)
        K = kc.camera(640, 480)
        cams = pose_cameras(K, *MOTIONS[kind], MB)
        mbf = float(cams[0]["mbf"])
        rng = np.random.default_rng(seed + 77)
        keys1 = k1["keys"].copy()
        keys1["octave"][rng.choice(len(keys1), 4, replace=False)] = [8, -1, 1 << 20, 9]
        k1 = dict(k1, keys=keys1)
        k3keys = k2["keys"].copy()
        k3keys["x"] += rng.uniform(-0.4, 0.4, len(k3keys)).astype(f32)
        k3keys["y"] += rng.uniform(-0.4, 0.4, len(k3keys)).astype(f32)
        sides = [with_depth(k1, mbf), with_depth(k2, mbf), with_depth(dict(k2, keys=k3keys), mbf)]
        raw = sides[0]["keys"].copy()
        raw["x"] += rng.uniform(-1, 1, len(raw)).astype(f32)
        sides[0]["keys_raw"] = raw
        pairs = [(0, 1), (0, 2)]
        match = [kc.oracle_triangulation(sides[a], sides[b], geo, lv[0], lv[1], 0, 1)[1] for a, b in pairs]
        _cache[key] = {"sides": sides, "cams": cams + [cams[1].copy()], "pairs": pairs, "match": match, "enabled": None, "levels": lv, "geo": geo,
                       "motion": MOTIONS[kind], "K": K}
    return _cache[key]


def random_cases():
    return {f"{kind}_{seed}": random_case(seed, kind) for kind in RANDOM_KINDS for seed in RANDOM_SEEDS}


# ---------------------------------------------------------------------------------------------------------------- feature counts

COUNTS = (0, 1, 63, 64, 65, 257, 300)  # an empty pair, one lane, either side of a wave, and of a work-group's chunk of 256


def count_case(n, n_sides=2, pairs=((0, 1),)):
    """n features per keyframe: world points seen from cameras 0.3 apart, the pixels moved by up to a pixel, 40 % stereo with depths that
    fit u_right, random octaves; feature i of keyframe 1 is matched to a random keyframe-2 feature (70 %: its own point) or to none"""
    key = ("count", n, n_sides, tuple(pairs))
    if key not in _cache:
        rng = np.random.default_rng(1000 + n)
        cams = [hand_cam((0.3 * k, 0.05 * k * k, 0.0), kc._rot(0.0, 0.02 * k, 0.0)) for k in range(n_sides)]
        P = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(2, 9, n)], 1)
        sides = []
        for cam in cams:
            uvz = np.array([project(cam, p) for p in P]).reshape(n, 3)
            xy = uvz[:, :2] + rng.uniform(-1, 1, (n, 2)) * (rng.random((n, 1)) < 0.5)
            ur = np.where(rng.random(n) < 0.4, xy[:, 0] - MBF / uvz[:, 2] + rng.uniform(-0.5, 0.5, n), -1.0)
            s = mk_side(xy, rng.integers(0, 8, n), ur)
            sides.append(with_depth(s, MBF))
        match = []
        for _ in pairs:
            row = np.where(rng.random(n) < 0.7, np.arange(n), rng.integers(0, max(n, 1), n))
            match.append(np.where(rng.random(n) < 0.8, row, -1).astype(np.int32))
        _cache[key] = {"sides": sides, "cams": cams, "pairs": list(pairs), "match": match, "enabled": None, "levels": HAND_LEVELS}
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------- the host forms

def host_expected(k1, k2s, cam1, cams2, levels, only_stereo=0, check_orientation=0):
    """what amos_match_new_points must return: geometry and gate per neighbour from the poses, the CPU oracle's search, the restatement
    over the neighbours that pass the gate -> (one NEW_POINT array per neighbour, NEW_POINTS_STATS [n2], the kept neighbours)"""
    sf, sg = levels
    kept, rows = [], []
    for v, (k2, c2) in enumerate(zip(k2s, cams2)):
        geo, ok = nr.pair_geometry(cam1, c2)
        if ok:
            kept.append(v)
            rows.append(kc.oracle_triangulation(k1, k2, geo, sf, sg, only_stereo, check_orientation)[1])
    new, stats = [np.zeros(0, nr.NEW_POINT) for _ in k2s], np.zeros(len(k2s), nr.NEW_POINTS_STATS)
    if kept:
        res = nr.new_points([k1] + [k2s[v] for v in kept], [cam1] + [cams2[v] for v in kept], [(0, i + 1) for i in range(len(kept))], rows, levels)
        for v, (rec, _, st) in zip(kept, res):
            new[v], stats[v] = rec, st
    return new, stats, kept


# ---------------------------------------------------------------------------------------------------------------- synth keyframes

SYNTH = (160, 120, 300, 4)  # width, height, features, levels


def synth_case(ob, synth):
    """Four 160 x 120 frames of the synth stream (frame k: the scene moved by (2 k, k) pixels) as keyframes: FeatureVectors at levelsup 2,
    30 % with a map point, 40 % stereo with depths from u_right, kc.PAIRS with the shift geometries and cameras whose poses give them."""
    if "synth" not in _cache:
        import bow_restatement as br
        w, h, nf, nl = SYNTH
        orc = ob.Oracle(nf, 1.2, nl)
        rng = np.random.default_rng(160)
        K = kc.camera(w, h)
        Kt = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        mbf = MB * K[0, 0]
        sides = []
        for k in range(4):
            kps, desc = orc.extract(synth.frame(3, k, h, w))
            n = len(kps)
            s = kc.side(desc, kps["angle"], br.transform(bc.vocabulary(), desc, 2)["fv"], (rng.random(n) < 0.3).astype(np.uint8))
            s["keys"] = kps.copy()
            s["u_right"] = np.where(rng.random(n) < 0.4, kps["x"] - rng.uniform(1, 8, n), -1.0).astype(f32)
            sides.append(with_depth(s, mbf))
        # frame k sees the scene (a plane at depth 1) moved by (-2 k, -k) pixels: camera k stands at k * (2 / fx, 1 / fy, 0)
        step = np.array([2.0 / K[0, 0], 1.0 / K[1, 1], 0.0])
        cams = [nr.camera(np.eye(3), -k * step, Kt, 0.001, 0.001 * K[0, 0], 1.2) for k in range(4)]
        _cache["synth"] = {"sides": sides, "cams": cams, "pairs": list(kc.PAIRS), "levels": kc.levels(nl), "enabled": None}
    return _cache["synth"]


# ---------------------------------------------------------------------------------------------------------------- the checks

def check_cases():
    """asserts that the cases do what they are named for (in the restatement); returns the verdict histogram of the random cases"""
    hand = hand_cases()
    for name, case in hand.items():
        assert all(len(s["keys"]) <= 2 for s in case["sides"]) and max(len(s["keys"]) for s in case["sides"]) + 1 <= CAPACITY, name
        res = run_case(case)
        for p, (new, verdicts, stats) in enumerate(res):
            assert verdicts.tolist() == case["expect"][p], (name, p, verdicts.tolist())
            assert int(stats["status"]) == case["status"][p], (name, p)
            assert int(stats["n_new"]) == len(new) == sum(v <= nr.UNPROJECTED_2 for v in verdicts if v >= 0), name

    def one(name, **change):
        case = hand[name]
        s1, s2 = case["sides"][0], case["sides"][1]
        tr = {}
        c1, c2 = change.get("c1", case["cams"][0]), change.get("c2", case["cams"][1])
        v, X = nr.triangulate_match(c1, c2, nr.feature(change.get("s1", s1), 0), nr.feature(s2, 0), *case["levels"], trace=tr)
        return v, X, tr
    # the two ways into LOW_PARALLAX
    assert float(one("low_parallax_small_angle")[2]["cos_rays"]) >= 0.9998 and one("low_parallax_cos_negative")[2]["cos_rays"] <= 0
    # :458: with cosParallaxStereo2 computed as well the verdict would have been UNPROJECTED_2
    v, _, tr = one("both_stereo_else_if")
    cs2 = nr.cos_stereo_parallax(MB, 4.0)
    assert v == nr.TRIANGULATED and cs2 < tr["cos_rays"] < tr["cs1"] and tr["cs2"] == tr["cos_rays"] + f32(1.0)
    # :563: with keyframe 2's own mbf the second gate passes
    case = hand["reprojection_2_other_mbf"]
    v, X, _ = one("reprojection_2_other_mbf")
    c1, c2, f2, sg = case["cams"][0], case["cams"][1], nr.feature(case["sides"][1], 0), case["levels"][1][0]
    assert v == nr.REPROJECTION_2 and c1["mbf"] != c2["mbf"]
    assert nr.view_gates(c2, f2, True, c1["mbf"], sg, X) == 2 and nr.view_gates(c2, f2, True, c2["mbf"], sg, X) == 0
    # KeyFrame.cc:816: the point comes from the raw keypoint
    case = hand["unprojected_1_raw_keys"]
    v_raw, X_raw, _ = one("unprojected_1_raw_keys")
    v_un, X_un, _ = one("unprojected_1_raw_keys", s1=dict(case["sides"][0], keys_raw=None))
    assert v_raw == v_un == nr.UNPROJECTED_1 and X_raw.tobytes() != X_un.tobytes()
    # :596, each side
    for name, below in (("scale_below", True), ("scale_above", False)):
        case = hand[name]
        sf = case["levels"][0]
        o1, o2 = int(case["sides"][0]["keys"]["octave"][0]), int(case["sides"][1]["keys"]["octave"][0])
        ratio_octave, ratio_factor = float(sf[o1]) / float(sf[o2]), 1.5 * 1.2
        assert (ratio_factor < ratio_octave) if below else (1.0 > ratio_octave * ratio_factor), name  # (the two distances are nearly equal)
    hist = np.zeros(nr.N_VERDICTS, np.int64)
    for name, case in random_cases().items():
        for new, verdicts, stats in run_case(case):
            hist += stats["n_verdict"]
    missing = [nr.VERDICT_NAMES[v] for v in range(nr.N_VERDICTS) if v not in (nr.W_ZERO, nr.DISTANCE_ZERO) and hist[v] == 0]
    assert not missing, (missing, hist.tolist())
    return hist
