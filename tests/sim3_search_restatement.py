"""ORBmatcher::SearchBySim3 (ORBmatcher.cc:1314-1555) restated feature by feature in plain Python / numpy for the tests, as
include/amos_frontend.h ("loop-closing Sim3 search") defines the arithmetic -- float32 operation by operation, float64 where OpenCV's gemm
and cv::norm use it: the row pass of :1347-1357, the two directions (:1367-1449, :1456-1533) in the reference's order over a grid built as
Frame::AssignFeaturesToGrid builds it (tests/fuse_restatement.py's Grid: KeyFrame::GetFeaturesInArea), and the agreement over i1
(:1539-1552).  Also the one seeded scene the CPU and GPU tests share."""
import functools

import numpy as np

import fuse_restatement as fr
import local_points_restatement as lr

f32, f64 = np.float32, np.float64
MAP_POINT = lr.MAP_POINT
KP = lr.hb.KP
CAMERA = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])  # amos_sim3_camera
PAIR = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("th", "<f4"), ("enabled", "<i4")])            # amos_sim3_search_pair
STATS = ("n_found", "n_in_view_12", "n_in_view_21", "n_single_12", "n_single_21", "skipped", "code", "pad")
REASONS = {"no_point": 1, "matched": 2, "behind": 3, "image": 4, "near": 5, "far": 6, "empty": 7, "none": 8, "accepted": 9}
MATCHED_ELSEWHERE = -2
TH_HIGH = 100
SCALE = lr.HAND_SCALE
BOUNDS = (0.0, 640.0, 0.0, 480.0)
FX = FY = 512.0
CX, CY = 320.0, 240.0  # u = 512 x + 320 is exact for x = +-0.625: the image's left and right bounds


def hops(R12, t12, s12):
    """-> (sR12, t12), (sR21, t21) (:1333-1335)"""
    R12, t12 = np.asarray(R12, f32).reshape(3, 3), np.asarray(t12, f32).reshape(3)
    s = f64(f32(s12))
    with np.errstate(all="ignore"):
        inv = f64(1.0) / s
        sR12 = np.array([[f32(s * f64(R12[r, c])) for c in range(3)] for r in range(3)], f32)
        sR21 = np.array([[f32(inv * f64(R12[c, r])) for c in range(3)] for r in range(3)], f32)
        t21 = np.array([f32(-((f64(sR21[r, 0]) * f64(t12[0]) + f64(sR21[r, 1]) * f64(t12[1])) + f64(sR21[r, 2]) * f64(t12[2]))) for r in range(3)], f32)
    return (sR12, t12.copy()), (sR21, t21)


def gemm(R, t, P):
    """R * P + t: per row ((R0 P0 + R1 P1) + R2 P2) + t in double, one rounding"""
    R, t, P = np.asarray(R, f32).reshape(3, 3).astype(f64), np.asarray(t, f32).astype(f64), np.asarray(P, f32).astype(f64)
    return np.array([f32(((R[r, 0] * P[0] + R[r, 1] * P[1]) + R[r, 2] * P[2]) + t[r]) for r in range(3)], f32)


def project(cam_from, hop, cam1, point, scale_factors, bounds):
    """One point through its keyframe's pose and the hop, with KF1's intrinsics -> (reason or 0, u, v, level)"""
    sf = np.asarray(scale_factors, f32)
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    with np.errstate(all="ignore"):
        pc = gemm(hop[0], hop[1], gemm(cam_from["Rcw"], cam_from["tcw"], point["pos"]))           # :1378-1379
        if pc[2] < f32(0):                                                                         # :1382
            return REASONS["behind"], f32(0), f32(0), 0
        invz = f32(1) / pc[2]                                                                      # :1386
        x, y = f32(pc[0] * invz), f32(pc[1] * invz)
        u = f32(f32(f32(cam1["fx"]) * x) + f32(cam1["cx"]))                                        # :1390-1391
        v = f32(f32(f32(cam1["fy"]) * y) + f32(cam1["cy"]))
        if not (u >= min_x and u < max_x and v >= min_y and v < max_y):                            # KeyFrame::IsInImage
            return REASONS["image"], f32(0), f32(0), 0
        d = pc.astype(f64)
        dist = f32(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))                             # :1399
        if dist < f32(f32(0.8) * f32(point["min_distance"])):                                      # :1402
            return REASONS["near"], f32(0), f32(0), 0
        if dist > f32(f32(1.2) * f32(point["max_distance"])):
            return REASONS["far"], f32(0), f32(0), 0
        level = int(lr.table_level(f32(point["max_distance"]) / dist, sf))                         # :1407
    return 0, u, v, level


def direction(src, dst, dst_grid, dst_bits, cam_from, hop, cam1, th, matched, scale_factors, bounds, infos=None):
    """One of the two loops -> (vnMatch [n_src], reason, u, v, level per source feature)"""
    sf = np.asarray(scale_factors, f32)
    n = len(src["kps"])
    match, reason = np.full(n, -1, np.int32), np.zeros(n, np.int8)
    us, vs, levels = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, np.int32)
    dkps = dst["kps"]
    for i in range(n):
        p = src["points"][i]
        if p["flags"] & lr.SKIP:                                                                   # !pMP, isBad()
            reason[i] = REASONS["no_point"]
            continue
        if matched[i]:
            reason[i] = REASONS["matched"]
            continue
        why, u, v, level = project(cam_from, hop, cam1, p, sf, bounds)
        if why:
            reason[i] = why
            continue
        us[i], vs[i], levels[i] = u, v, level
        cand = dst_grid.area(dkps, u, v, f32(f32(th) * sf[level])) if len(dkps) else []           # :1411-1414
        if infos is not None:
            infos.append(dict(feature=i, columns=len({c // fr.ROWS for _, c in cand}), cells=len({c for _, c in cand}), r=float(f32(th) * sf[level]),
                              u=float(u), v=float(v), tie=False, best=256))
        if not cand:
            reason[i] = REASONS["empty"]
            continue
        qbits = np.unpackbits(p["desc"])
        best_dist, best_idx, cells_at_best = 1 << 30, -1, set()
        for idx, cell in cand:
            octave = int(dkps["octave"][idx])
            if octave < level - 1 or octave > level:                                              # :1431
                continue
            dist = int((dst_bits[idx] != qbits).sum())
            if dist < best_dist:                                                                   # :1438
                best_dist, best_idx, cells_at_best = dist, idx, {cell}
            elif dist == best_dist:
                cells_at_best.add(cell)
        if infos is not None:
            infos[-1]["tie"], infos[-1]["best"] = best_dist <= TH_HIGH and len(cells_at_best) > 1, min(best_dist, 256)
        if best_dist <= TH_HIGH:                                                                   # :1445
            match[i] = best_idx
            reason[i] = REASONS["accepted"]
        else:
            reason[i] = REASONS["none"]
    return match, reason, us, vs, levels


_GRIDS = {}


def grid_and_bits(kf, bounds):
    """the keyframe's grid (kept per keyframe: the pairs of the scene share a few) and its descriptors as bits"""
    key = (kf["kps"].tobytes(), tuple(float(b) for b in bounds))
    if key not in _GRIDS:
        _GRIDS[key] = fr.Grid(kf["kps"], bounds)
    return _GRIDS[key], np.unpackbits(np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32), axis=1)


def search(kf1, kf2, cam1, cam2, R12, t12, s12, th, row, scale_factors, bounds, with_infos=False):
    """kf: dict(kps [n], desc [n][32], points [n] MAP_POINT); row: int32 [n1].  -> dict(match_out, match1, match2, stats (dict), and per
    direction reason / u / v / level / infos)"""
    n1, n2 = len(kf1["kps"]), len(kf2["kps"])
    row = np.asarray(row, np.int32)
    matched1, matched2 = np.zeros(n1, bool), np.zeros(n2, bool)
    for i in range(n1):                                                                            # :1347-1357
        if row[i] != -1:
            matched1[i] = True
            if 0 <= row[i] < n2:
                matched2[row[i]] = True
    h12, h21 = hops(R12, t12, s12)
    g1, b1 = grid_and_bits(kf1, bounds)
    g2, b2 = grid_and_bits(kf2, bounds)
    i12, i21 = ([], []) if with_infos else (None, None)
    m1, why1, u1, v1, l1 = direction(kf1, kf2, g2, b2, cam1, h21, cam1, th, matched1, scale_factors, bounds, i12)
    m2, why2, u2, v2, l2 = direction(kf2, kf1, g1, b1, cam2, h12, cam1, th, matched2, scale_factors, bounds, i21)
    out = row.copy()
    found = 0
    for i1 in range(n1):                                                                           # :1539-1552
        idx2 = m1[i1]
        if idx2 >= 0 and m2[idx2] == i1:
            out[i1] = idx2
            found += 1
    seen = lambda why: int((why >= REASONS["empty"]).sum())
    stats = dict(n_found=found, n_in_view_12=seen(why1), n_in_view_21=seen(why2), n_single_12=int((m1 >= 0).sum()), n_single_21=int((m2 >= 0).sum()),
                 skipped=0, code=0, pad=0)
    return dict(match_out=out, match1=m1, match2=m2, stats=stats, reason=(why1, why2), u=(u1, u2), v=(v1, v2), level=(l1, l2), infos=(i12, i21),
                matched=(matched1, matched2))


def stats_row(stats):
    return np.array([stats[k] for k in STATS], np.int32)


# ---------------------------------------------------------------------------------------------------------------- the shared scene

CAPACITY = 603     # no multiple of a block's 32 features: the last block of a row is partly filled
SIZES = (0, 37, 300, 600, 257, 31, 33)
MAP_SCALE = (1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0)  # keyframe 4's map is the scene at twice the size: s12 = 0.5 and 2 against keyframe 3
N_DUP = 10
POISON = -7


def camera_of(R, t):
    c = np.zeros((), CAMERA)
    c["Rcw"], c["tcw"] = np.asarray(R, f32).reshape(9), np.asarray(t, f32)
    c["fx"], c["fy"], c["cx"], c["cy"] = FX, FY, CX, CY
    return c


def _pixel(R, t, X):
    q = X @ R.astype(f64).T + t.astype(f64)
    return FX * q[:, 0] / q[:, 2] + CX, FY * q[:, 1] / q[:, 2] + CY, q


def _hand_points(rng):
    """Points of keyframe 2 (identity pose) for the pair (2, 2) with the identity Sim3 -> [(name, MAP_POINT)]"""
    rows = []

    def add(name, pos, min_d=0.5, max_d=None):
        p = np.zeros((), MAP_POINT)
        p["pos"] = pos
        p["min_distance"], p["max_distance"] = min_d, (max_d if max_d is not None else 1.1 * float(np.linalg.norm(pos)))
        p["desc"] = rng.integers(0, 256, 32, dtype=np.uint8)
        rows.append((name, p))
    add("u_min", (-0.625 * 2, 0.0, 2.0))                                      # u == min_x exactly: in
    add("u_max", (0.625 * 2, 0.0, 2.0))                                       # u == max_x exactly: out
    lo, hi = f32(f32(0.8) * f32(2.3)), f32(f32(1.2) * f32(1.9))
    add("band_lo_in", (0.0, 0.0, lo), min_d=2.3, max_d=4.1)                   # dist3D == 0.8f * min_distance: in
    add("band_lo_out", (0.0, 0.0, np.nextafter(lo, f32(0))), min_d=2.3, max_d=4.1)
    add("band_hi_in", (0.0, 0.0, hi), min_d=0.5, max_d=1.9)                   # dist3D == 1.2f * max_distance: in
    add("band_hi_out", (0.0, 0.0, np.nextafter(hi, f32(9))), min_d=0.5, max_d=1.9)
    add("behind", (0.1, 0.1, -1.0))
    add("z_zero", (0.3, 0.2, 0.0))                                            # the projection is infinite: out of the image
    for name, (u, v) in HAND_SPOTS.items():
        z = 2.0
        add(name, ((u - CX) / FX * z, (v - CY) / FY * z, z))                  # level 1 (ratio 1.1): radius 9, octaves 0 .. 1
    return rows


# name -> the pixel a hand point projects to; its target feature sits there (the tie's two at x = 254 and x = 256, either side of a cell border)
HAND_SPOTS = {"dist_100": (50.0, 430.0), "dist_101": (150.0, 430.0), "tie": (255.0, 430.0), "dist_60": (400.0, 430.0), "dist_0": (520.0, 430.0)}
HAND_TARGETS = (("dist_100", 50.0, 100), ("dist_101", 150.0, 101), ("dist_60", 400.0, 60), ("dist_0", 520.0, 0), ("tie", 256.0, 7), ("tie", 254.0, 7))
BAD = 4  # beside lr.SKIP in a point's flags: the feature has a point and it isBad() (the device reads bit 0 only)


def scene(seed=23):
    """7 keyframe slots of 0 / 37 / 300 / 600 / 257 / 31 / 33 features at a capacity of 603 over one physical scene of 590 points; every keyframe
    owns the map points of its features (its own map, keyframe 4's at twice the size).  Keyframe 3 sees every point, and its last ten
    features see the first ten points again.  Keyframe 2 has the identity pose and carries the hand points for the pair (2, 2).
    -> dict(kps, desc, points [7][603], counts, cameras, pairs (PAIR records), slots1, slots2, rows [pairs][603], kinds, ...)"""
    rng = np.random.default_rng(seed)
    sf = SCALE.astype(f64)
    n_levels = len(sf)
    n_phys = SIZES[3] - N_DUP
    eye = np.eye(3)
    poses = [lr.pose(0.0, 0.0, 0.0, [0, 0, 0]), lr.pose(0.02, -0.03, 0.01, [0.1, -0.05, 0.05]), (eye.astype(f32), np.zeros(3, f32)),
             lr.pose(-0.02, 0.04, -0.015, [-0.12, 0.06, 0.08]), lr.pose(0.03, 0.02, 0.02, [0.08, 0.1, -0.06]),
             lr.pose(-0.01, -0.02, 0.0, [0.05, 0.02, 0.1]), lr.pose(0.015, 0.03, -0.02, [-0.06, -0.08, 0.04])]
    # the physical scene: random pixels of keyframe 3 at seeded depths, each with a level (the octave it is seen at) and a descriptor
    R3, t3 = poses[3][0].astype(f64), poses[3][1].astype(f64)
    pix = np.stack([rng.uniform(4, 636, n_phys), rng.uniform(4, 476, n_phys)], 1)
    pix[:N_DUP] = np.stack([rng.uniform(200, 440, N_DUP), rng.uniform(150, 330, N_DUP)], 1)  # the doubled points: in every keyframe's image
    depth = rng.uniform(2.0, 8.0, n_phys)
    q3 = np.stack([(pix[:, 0] - CX) / FX * depth, (pix[:, 1] - CY) / FY * depth, depth], 1)
    X = (q3 - t3) @ R3
    level = rng.integers(0, n_levels, n_phys)
    level[:N_DUP] = rng.integers(4, n_levels, N_DUP)
    base = rng.integers(0, 256, (n_phys, 32), dtype=np.uint8)
    hand = _hand_points(rng)
    spots = np.array(list(HAND_SPOTS.values()))

    kps = np.zeros((len(SIZES), CAPACITY), KP)
    desc = np.zeros((len(SIZES), CAPACITY, 32), np.uint8)
    points = np.zeros((len(SIZES), CAPACITY), MAP_POINT)
    points["flags"] = lr.SKIP
    phys_of = np.full((len(SIZES), CAPACITY), -1, np.int64)  # the physical point a feature sees
    hand_at = {}
    for f, n in enumerate(SIZES):
        if n == 0:
            continue
        R, t = poses[f][0].astype(f64), poses[f][1].astype(f64)
        u, v, q = _pixel(R, t, X)
        visible = (u >= 3) & (u < 637) & (v >= 3) & (v < 477) & (q[:, 2] > 0.5)
        if f == 2:  # nothing of the scene near the hand spots
            for su, sv in spots:
                visible &= ~((np.abs(u - su) < 60) & (np.abs(v - sv) < 45))
        n_hand = len(hand) + len(HAND_TARGETS) if f == 2 else 0
        n_reg = n - n_hand - (N_DUP if f == 3 else 0)
        must = np.arange(N_DUP)
        assert visible[must].all(), f
        rest = rng.permutation(np.nonzero(visible & (np.arange(n_phys) >= N_DUP))[0])[:n_reg - N_DUP]
        ids = rng.permutation(np.concatenate([must, rest]))
        assert len(ids) == n_reg, (f, len(ids), n_reg)
        if f == 3:
            ids = np.concatenate([ids, must])  # the last ten features see the first ten points again
        m = len(ids)
        noise = rng.normal(0, 0.7, (m, 2)) * sf[level[ids], None]
        k = kps[f]
        k["x"][:m], k["y"][:m] = np.clip(u[ids] + noise[:, 0], 0.5, 639.4), np.clip(v[ids] + noise[:, 1], 0.5, 479.4)
        k["octave"][:m], k["size"][:m], k["angle"][:m] = level[ids], 31, rng.uniform(0, 360, m)
        phys_of[f, :m] = ids
        dist = np.linalg.norm(q[ids], axis=1)
        if f == 4:
            # its octaves follow the level keyframe 3's points predict inside keyframe 4's map (dist3D is twice the physical distance)
            ratio4 = sf[level[ids]] * 0.96 / MAP_SCALE[4]
            k["octave"][:m] = np.minimum((ratio4[:, None] > sf[None, :]).sum(1), n_levels - 1)
        for j, pid in enumerate(ids):
            desc[f, j] = fr.flip_bits(rng, base[pid], int(rng.integers(0, 12)))
        # the keyframe's own map points: 70 % of its features carry one, a few of them bad
        has = rng.random(m) < 0.7
        has[np.isin(ids, must)] = True
        p = points[f]
        p["pos"][:m] = (MAP_SCALE[f] * X[ids]).astype(f32)
        p["normal"][:m] = (0, 0, 1)
        # max_distance in the PARTNER's map units (keyframe 4 is only ever paired with keyframe 3): the level of a partner at about the same distance
        p["max_distance"][:m] = (dist * sf[level[ids]] * rng.uniform(0.94, 0.98, m)).astype(f32)
        p["min_distance"][:m] = (p["max_distance"][:m] / sf[-1] / 1.5).astype(f32)
        gate = rng.random(m)
        gate[np.isin(ids, must)] = 1.0
        far, near, bad = gate < 0.04, (gate >= 0.04) & (gate < 0.08), (gate >= 0.08) & (gate < 0.12)
        p["max_distance"][:m] = np.where(far, dist / 1.3, np.where(near, dist * 3, p["max_distance"][:m])).astype(f32)
        p["min_distance"][:m] = np.where(near, dist * 1.4, np.where(far, dist / 10, p["min_distance"][:m])).astype(f32)
        p["flags"][:m] = np.where(~has, lr.SKIP, np.where(bad, lr.SKIP | BAD, 0))
        for j, pid in enumerate(ids):
            p["desc"][j] = fr.flip_bits(rng, base[pid], int(rng.integers(0, 12)))
        if f == 2:
            # the hand block: a source feature per hand point (its own keypoint is a stray one), then the four target features
            for j, (name, hp) in enumerate(hand):
                i = m + j
                k["x"][i], k["y"][i], k["octave"][i], k["size"][i] = rng.uniform(300, 620), rng.uniform(20, 60), 7, 31
                desc[f, i] = rng.integers(0, 256, 32, dtype=np.uint8)
                points[f, i] = hp
                hand_at[name] = i
            tgt = m + len(hand)
            by = dict(hand)
            last = len(HAND_TARGETS) - 1
            for i, (name, x, bits) in enumerate(HAND_TARGETS):
                k["x"][tgt + i], k["y"][tgt + i], k["octave"][tgt + i], k["size"][tgt + i] = x, 430.0, 1, 31
                desc[f, tgt + i] = fr.flip_bits(rng, by[name]["desc"], bits) if i < last else desc[f, tgt + last - 1]  # the tie's second: a copy
                hand_at["target_" + name + ("_b" if i == last else "")] = tgt + i
    counts = np.array(SIZES, np.int32)
    cameras = np.array([camera_of(R, f32(MAP_SCALE[f]) * t) for f, (R, t) in enumerate(poses)], CAMERA)

    def truth(a, b):
        """the Sim3 with p_c1 = s12 R12 p_c2 + t12 for keyframes a, b of map scales sa, sb"""
        Ra, ta, Rb, tb = (x.astype(f64) for x in (*poses[a], *poses[b]))
        R12 = Ra @ Rb.T
        return R12, MAP_SCALE[a] * (ta - R12 @ tb), MAP_SCALE[a] / MAP_SCALE[b]

    def turned(R12, t12, s12, rx, ry, dt):
        Rp, _ = lr.pose(rx, ry, 0.0, [0, 0, 0])
        return Rp.astype(f64) @ R12, t12 + np.asarray(dt), s12

    flip = np.diag([-1.0, 1.0, -1.0])  # half a turn about y: every point of the other keyframe lies behind the camera
    specs = [("truth", 3, 2, truth(3, 2), 7.5), ("other_sim3", 3, 2, turned(*truth(3, 2), 0.004, -0.003, [0.004, -0.003, 0.002]), 7.5),
             ("same", 2, 2, (eye, np.zeros(3), 1.0), 7.5), ("empty_1", 0, 3, truth(0, 3), 7.5), ("empty_2", 3, 0, truth(3, 0), 7.5),
             ("half", 3, 4, truth(3, 4), 7.5), ("double", 4, 3, truth(4, 3), 7.5), ("wide", 1, 3, truth(1, 3), 40.0),
             ("n31", 5, 3, truth(5, 3), 7.5), ("n33", 6, 3, truth(6, 3), 7.5), ("behind", 3, 2, (flip @ truth(3, 2)[0], truth(3, 2)[1], 1.0), 7.5)]
    degenerate = {"empty_1", "empty_2", "behind"}
    pairs = np.zeros(len(specs), PAIR)
    rows = np.full((len(specs), CAPACITY), POISON, np.int32)
    for p, (name, a, b, (R12, t12, s12), th) in enumerate(specs):
        pairs[p]["R12"], pairs[p]["t12"], pairs[p]["s12"], pairs[p]["th"], pairs[p]["enabled"] = np.asarray(R12, f32).reshape(9), t12, s12, th, 1
        n1, n2 = SIZES[a], SIZES[b]
        row = np.full(n1, -1, np.int32)
        where = {int(pid): j for j, pid in enumerate(phys_of[b, :n2]) if pid >= 0}
        share = 0.12 if n1 < 100 else 0.3
        for i in range(n1):
            pid = int(phys_of[a, i])
            if pid < N_DUP or points[a, i]["flags"] & lr.SKIP or rng.random() >= share:  # (the hand block and the doubled points stay free)
                continue
            kind = rng.random()
            row[i] = where[pid] if pid in where and kind < 0.8 else (MATCHED_ELSEWHERE if kind < 0.93 else n2 + int(rng.integers(0, 9)))
        rows[p, :n1] = row
    return dict(kps=kps, desc=desc, points=points, counts=counts, cameras=cameras, pairs=pairs, slots1=np.array([s[1] for s in specs], np.int32),
                slots2=np.array([s[2] for s in specs], np.int32), rows=rows, names=[s[0] for s in specs], degenerate=degenerate, hand=hand_at,
                phys_of=phys_of, sf=SCALE, bounds=BOUNDS, capacity=CAPACITY)


def keyframe(sc, f, n=None):
    n = int(sc["counts"][f]) if n is None else n
    return dict(kps=sc["kps"][f, :n], desc=sc["desc"][f, :n], points=sc["points"][f, :n])


def run_pair(sc, p, with_infos=False, pair=None, row=None, counts=None):
    """the restatement on pair p of the scene (optionally with another Sim3 record, row or count array)"""
    a, b = int(sc["slots1"][p]), int(sc["slots2"][p])
    pr = sc["pairs"][p] if pair is None else pair
    counts = sc["counts"] if counts is None else counts
    n1 = min(int(counts[a]), sc["capacity"])
    row = sc["rows"][p] if row is None else row
    return search(keyframe(sc, a, n1), keyframe(sc, b, min(int(counts[b]), sc["capacity"])), sc["cameras"][a], sc["cameras"][b], pr["R12"], pr["t12"],
                  pr["s12"], pr["th"], row[:n1], sc["sf"], sc["bounds"], with_infos)


@functools.lru_cache(maxsize=None)
def shared():
    """(scene, [the restatement's result per pair, with infos]): computed once per session and left unchanged"""
    sc = scene()
    return sc, [run_pair(sc, p, with_infos=True) for p in range(len(sc["pairs"]))]


def expected_arrays(sc, results, rows_in=None, skip=()):
    """What the batch entry leaves for all pairs: (match_out, match1, match2 [pairs][capacity], stats [pairs][8]).  Rows from N1 on are the
    input's, match1 / match2 are -1 from N1 / N2 on; pairs in `skip` keep `rows_in` / POISON and are not filled here."""
    n, cap = len(results), sc["capacity"]
    out = (sc["rows"] if rows_in is None else rows_in).copy()
    m1, m2, stats = np.full((n, cap), -1, np.int32), np.full((n, cap), -1, np.int32), np.zeros((n, 8), np.int32)
    for p, r in enumerate(results):
        if p in skip:
            m1[p], m2[p] = POISON, POISON
            continue
        out[p, :len(r["match_out"])] = r["match_out"]
        m1[p, :len(r["match1"])], m2[p, :len(r["match2"])] = r["match1"], r["match2"]
        stats[p] = stats_row(r["stats"])
    return out, m1, m2, stats
