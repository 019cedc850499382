"""ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:388-512) and the count of LoopClosing.cc:538-546 restated
for the tests in plain Python / numpy exactly as include/amos_frontend.h ("loop-closing point search") defines them: Scw's decomposition
(tests/adaptor_prefilter.py unscaled / centre), the pre-filter float32 operation by operation (float64 where the definition says so),
KeyFrame::GetFeaturesInArea over the 64 x 48 grid, and ONE sequential loop over the points with a set of occupied features.  Also the
ONE seeded scene the CPU and GPU tests share, and the hand-made greedy case."""
import numpy as np

import adaptor_prefilter as ap
import fuse_restatement as fr
import local_points_restatement as lr

f32, f64 = np.float32, np.float64
MAP_POINT = lr.MAP_POINT
SKIP = lr.SKIP
QUERY = np.dtype([("Scw", "<f4", (16,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("th", "<f4"), ("frame", "<i4"),
                  ("max_dist", "<i4"), ("min_inliers", "<i4"), ("min_total", "<i4"), ("enabled", "<i4"), ("found_from_match", "<i4")])
STATS = ("n_candidates", "n_in_view", "n_matches", "n_researched", "n_total", "accepted", "status", "skipped")
REASONS = {"bad": 1, "found": 2, "behind": 3, "image": 4, "near": 5, "far": 6, "angle": 7}
MATCHED_ELSEWHERE = -2
SCALE, BOUNDS = fr.SCALE, fr.BOUNDS
INTR = (512.0, 512.0, 250.0, 240.0)


def query(frame, Scw, intr=INTR, th=10.0, max_dist=50, min_inliers=20, min_total=40, enabled=1, found_from_match=0):
    q = np.zeros((), QUERY)
    q["Scw"] = np.asarray(Scw, f32).reshape(16)
    q["fx"], q["fy"], q["cx"], q["cy"] = intr
    q["th"], q["frame"], q["max_dist"], q["min_inliers"], q["min_total"] = th, frame, max_dist, min_inliers, min_total
    q["enabled"], q["found_from_match"] = enabled, found_from_match
    return q


def decompose(Scw):
    """-> (Rcw [3, 3], tcw, Ow) of :397-403"""
    R, t = ap.unscaled(np.asarray(Scw, f32).reshape(4, 4))
    return R, t, ap.centre(R, t)


def found_of(n_features, n_points, q, matched, found, point_of_feature2):
    """spAlreadyFound as one flag per point of the query: the caller's bytes, and with found_from_match the points the entry row names"""
    fd = np.zeros(n_points, bool) if found is None else np.asarray(found) != 0
    fd = fd.copy()
    if int(q["found_from_match"]):
        pf2 = np.asarray(point_of_feature2)
        for i in range(n_features):
            j = int(matched[i])
            if 0 <= j < len(pf2) and 0 <= int(pf2[j]) < n_points:
                fd[int(pf2[j])] = True
    return fd


def prefilter(points, fd, Scw, q, scale_factors, bounds):
    """:416-462 -> (u, v, level per point: zeros where not in view; in_view bool; reason per point, 0 in view; status)"""
    sf = np.asarray(scale_factors, f32)
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    n = len(points)
    u_, v_, level = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, np.int32)
    in_view, reason = np.zeros(n, bool), np.zeros(n, np.int8)
    Rf, tf, Ow = decompose(Scw)
    R, t = Rf.astype(f64), tf.astype(f64)
    fx, fy, cx, cy = (f32(q[k]) for k in ("fx", "fy", "cx", "cy"))
    status = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            if points["flags"][i] & SKIP:                                                                 # :419
                reason[i] = REASONS["bad"]
                continue
            if fd[i]:                                                                                     # :420
                reason[i] = REASONS["found"]
                continue
            P = points["pos"][i].astype(f32)
            Pd = P.astype(f64)
            Pc = [f32(((R[r, 0] * Pd[0] + R[r, 1] * Pd[1]) + R[r, 2] * Pd[2]) + t[r]) for r in range(3)]  # :427
            if Pc[2] < f32(0):                                                                            # :430
                reason[i] = REASONS["behind"]
                continue
            invz = f32(1) / Pc[2]                                                                         # :434
            x, y = f32(Pc[0] * invz), f32(Pc[1] * invz)
            u, v = f32(f32(fx * x) + cx), f32(f32(fy * y) + cy)                                           # :438-439
            if not (u >= min_x and u < max_x and v >= min_y and v < max_y):                               # KeyFrame::IsInImage
                reason[i] = REASONS["image"]
                if not (np.isfinite(u) and np.isfinite(v)):
                    status |= 1
                continue
            PO = (P - Ow).astype(f32)
            POd = PO.astype(f64)
            dist = f32(np.sqrt((POd[0] * POd[0] + POd[1] * POd[1]) + POd[2] * POd[2]))                    # :449
            lo, hi = f32(f32(0.8) * points["min_distance"][i]), f32(f32(1.2) * points["max_distance"][i])
            if dist < lo or dist > hi:                                                                    # :451
                reason[i] = REASONS["near"] if dist < lo else REASONS["far"]
                continue
            Pn = points["normal"][i].astype(f64)
            if ((POd[0] * Pn[0] + POd[1] * Pn[1]) + POd[2] * Pn[2]) < 0.5 * f64(dist):                    # :457
                reason[i] = REASONS["angle"]
                continue
            u_[i], v_[i], level[i] = u, v, lr.table_level(f32(points["max_distance"][i]) / dist, sf)      # :460
            in_view[i] = True
    return u_, v_, level, in_view, reason, status


def skipped_result(n_features):
    out = dict(loop_match=np.full(n_features, -1, np.int32), infos={}, reason=None)
    out.update({k: 0 for k in STATS}, skipped=1)
    return out


def search(kps, desc, points, q, matched, found, point_of_feature2, scale_factors, bounds, Scw=None, opt=None):
    """One query.  matched [len(kps)]: vpMatched on entry (-1 free, everything else occupied); found [len(points)] or None;
    point_of_feature2 or None; Scw: in place of the record's; opt: dict(skipped, code, n_inliers, Scw) of the optimiser's row, or None.
    -> dict(loop_match [len(kps)], every field of amos_loop_points_stats, reason per point, infos: per point in view what the tests' case
    counts read)."""
    points = np.ascontiguousarray(points, MAP_POINT)
    n = len(kps)
    matched = np.asarray(matched, np.int32)
    assert len(matched) == n
    if not int(q["enabled"]) or (opt is not None and (opt["skipped"] != 0 or opt["code"] != 0 or opt["n_inliers"] < int(q["min_inliers"]))):
        return skipped_result(n)
    S = opt["Scw"] if opt is not None else (q["Scw"] if Scw is None else Scw)
    sf = np.asarray(scale_factors, f32)
    fd = found_of(n, len(points), q, matched, found, point_of_feature2)
    u, v, level, in_view, reason, status = prefilter(points, fd, S, q, sf, bounds)
    th, max_dist = f32(q["th"]), int(q["max_dist"])
    grid = fr.Grid(kps, bounds)
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1)
    on_entry = matched != -1
    occupied = set(int(i) for i in np.nonzero(on_entry)[0])
    loop_match = np.full(n, -1, np.int32)
    n_matches = n_researched = 0
    infos = {}
    for i in np.nonzero(in_view)[0]:                                                                      # the points in list order
        lvl = int(level[i])
        qbits = np.unpackbits(points["desc"][i])
        cand = []  # (distance, feature) in the reference's visiting order, behind the level gate
        for idx, _cell in grid.area(kps, u[i], v[i], f32(th * sf[lvl])):                                  # :464-470
            kl = int(kps["octave"][idx])
            if kl < lvl - 1 or kl > lvl:                                                                  # :486-487
                continue
            cand.append((int((bits[idx] != qbits).sum()), int(idx)))
        entry = sorted((c for c in cand if not on_entry[c[1]]), key=lambda c: c[0])[:2]  # stable: the first of equals
        best_dist, best = 256, -1
        for d, idx in cand:
            if idx in occupied:                                                                           # :482
                continue
            if d < best_dist:                                                                             # :491-495
                best_dist, best = d, idx
        info = dict(n_window=len(cand), occupied_on_entry=sum(1 for c in cand if on_entry[c[1]]), entry=entry, best_free=best_dist,
                    best_taken=bool(entry) and entry[0][1] in occupied, second_free=len(entry) == 2 and entry[1][1] not in occupied,
                    both_taken=len(entry) == 2 and entry[0][1] in occupied and entry[1][1] in occupied,
                    only_taken=len(entry) == 1 and entry[0][1] in occupied, accepted=False)
        # what the device counts: the window is searched again when both recorded features were near enough on entry and both are taken
        info["researched"] = info["both_taken"] and entry[1][0] <= max_dist
        n_researched += info["researched"]
        if best_dist <= max_dist:                                                                         # :498-502
            loop_match[best] = i
            occupied.add(best)
            n_matches += 1
            info["accepted"] = True
        infos[int(i)] = info
    n_total = int(on_entry.sum()) + n_matches                                                             # LoopClosing.cc:538-543
    return dict(loop_match=loop_match, n_candidates=int((reason >= REASONS["behind"]).sum() + in_view.sum()), n_in_view=int(in_view.sum()),
                n_matches=n_matches, n_researched=n_researched, n_total=n_total, accepted=int(n_total >= int(q["min_total"])), status=status,
                skipped=0, reason=reason, infos=infos, u=u, v=v, level=level, in_view=in_view)


# ---------------------------------------------------------------------------------------------------------------- the shared scene

def make_keyframe(rng, n_groups, isolated):
    """Features in tight groups of 1 .. 5 on one level, most of a group with near-identical descriptors (so that the points of a group
    contend for its features and a second or third choice is still within TH_LOW) and some with an unrelated one (a second choice that
    is not), then `isolated` single features far from any group."""
    xs, ys, octs, descs = [], [], [], []
    cols, rows = 16, 10
    cells = rng.permutation(cols * rows)
    for g in range(n_groups + isolated):
        c = int(cells[g])
        gx = BOUNDS[0] + 20 + (c % cols) * 38 + rng.uniform(0, 6)
        gy = BOUNDS[2] + 20 + (c // cols) * 44 + rng.uniform(0, 6)
        size = 1 if g >= n_groups else int(rng.integers(1, 6))
        octave = int(rng.integers(0, 2)) if g >= n_groups else int(rng.integers(0, len(SCALE)))  # a single feature's windows stay small
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for k in range(size):
            xs.append(gx + rng.uniform(-4, 4))
            ys.append(gy + rng.uniform(-4, 4))
            octs.append(octave)
            if k == 0:
                descs.append(base)
            elif rng.random() < 0.7:
                descs.append(fr.flip_bits(rng, base, int(rng.integers(0, 9))))
            else:  # a neighbour that looks like nothing in the group: a second choice far beyond TH_LOW
                descs.append(rng.integers(0, 256, 32, dtype=np.uint8))
    n = len(xs)
    kps = np.zeros(n, lr.hb.KP)
    kps["x"], kps["y"], kps["octave"], kps["size"] = np.array(xs, f32), np.array(ys, f32), octs, 31
    kps["angle"] = rng.uniform(0, 360, n)
    order = rng.permutation(n)  # the groups' members are not neighbours in feature order
    return kps[order], np.array(descs, np.uint8)[order]


def make_points(rng, kf, m, Scw, picks=None, gate_share=0.04, thresholds=()):
    """m loop points for one keyframe: features (drawn with replacement) back-projected through the unscaled Scw at seeded depths, a few
    descriptor bits flipped, max_distance for a predicted level at the feature's octave or one above; `gate_share` of them fail each
    pre-filter test.  thresholds: (point, feature, bits) -- that point sits on that feature with exactly `bits` descriptor bits flipped and
    passes every gate.  -> (points, the feature each was made from)"""
    kps, desc = kf
    pts = np.zeros(m, MAP_POINT)
    if m == 0:
        return pts, np.zeros(0, np.int64)
    R, t, Ow = (a.astype(f64) for a in decompose(Scw))
    fx, fy, cx, cy = INTR
    sf = SCALE.astype(f64)
    pick = rng.integers(0, len(kps), m) if picks is None else np.asarray(picks)
    gate = rng.random(m)
    for i, f, _ in thresholds:
        pick[i], gate[i] = f, 1.0
    k = kps[pick]
    du, dv = rng.normal(0, 0.8, m), rng.normal(0, 0.8, m)
    z = rng.uniform(2.0, 8.0, m)
    g = gate_share
    z = np.where(gate < g, -z, z)
    x = (k["x"].astype(f64) + du - cx) / fx * z
    y = (k["y"].astype(f64) + dv - cy) / fy * z
    x = np.where((gate >= g) & (gate < 2 * g), x + 3.0 * z, x)
    pts["pos"] = ((np.stack([x, y, z], 1) - t) @ R).astype(f32)
    PO = pts["pos"].astype(f64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    toward = PO / dist[:, None]
    side = np.cross(toward, rng.normal(0, 1, (m, 3)))
    side /= np.linalg.norm(side, axis=1)[:, None]
    away = (gate >= 2 * g) & (gate < 3 * g)
    normal = np.where(away[:, None], 0.2 * toward + side, toward + rng.normal(0, 0.15, (m, 3)))
    pts["normal"] = (normal / np.linalg.norm(normal, axis=1)[:, None]).astype(f32)
    lvl = np.minimum(k["octave"] + rng.integers(0, 2, m), len(sf) - 1)
    pts["max_distance"] = (dist * sf[lvl] * rng.uniform(0.93, 0.99, m)).astype(f32)
    pts["min_distance"] = (pts["max_distance"] / sf[-1] / 1.5).astype(f32)
    far, near = (gate >= 3 * g) & (gate < 4 * g), (gate >= 4 * g) & (gate < 5 * g)
    pts["max_distance"] = np.where(far, dist / 1.3, np.where(near, dist * 3, pts["max_distance"])).astype(f32)
    pts["min_distance"] = np.where(near, dist * 1.4, np.where(far, dist / 10, pts["min_distance"])).astype(f32)
    pts["flags"] = np.where((gate >= 5 * g) & (gate < 6 * g), SKIP, 0)
    for i in range(m):
        pts["desc"][i] = fr.flip_bits(rng, desc[pick[i]], int(rng.integers(0, 12)))
    for i, f, nbits in thresholds:
        pts["desc"][i] = fr.flip_bits(rng, desc[f], nbits)
    return pts, pick


def scw_of(scale, rx, ry, rz, t):
    R, tt = lr.pose(rx, ry, rz, t)
    S = np.eye(4, dtype=f32)
    S[:3, :3], S[:3, 3] = f32(scale) * R.astype(f32), f32(scale) * np.asarray(tt, f32)
    return S


N_ISOLATED = 24
N_LIST = (600, 40)


def scene(seed=6):
    """Two keyframes of about 300 features; a loop list of 600 points on keyframe 0 (eight per group: shared windows) and one of 40 on
    keyframe 1; Sim3s of scale 0.93 and 1.07.  Query 0 has found_from_match and is accepted, query 1 stays below min_total.  The last
    N_ISOLATED features of keyframe 0 (before the shuffle: found by position) are single; two of them carry the threshold points."""
    rng = np.random.default_rng(seed)
    kfs = [make_keyframe(rng, 100, N_ISOLATED), make_keyframe(rng, 100, N_ISOLATED)]
    S = [scw_of(0.93, 0.01, -0.02, 0.005, [0.05, -0.02, 0.1]), scw_of(1.07, -0.015, 0.01, -0.01, [-0.03, 0.04, -0.05])]
    kps0 = kfs[0][0]
    # single features of keyframe 0 on levels 0 and 1: no other feature inside any window around them (radius 10 * 1.2^2 at the most)
    apart = np.maximum(np.abs(kps0["x"][:, None] - kps0["x"][None, :]), np.abs(kps0["y"][:, None] - kps0["y"][None, :]))
    np.fill_diagonal(apart, 1e9)
    alone = np.nonzero((apart.min(1) > 18.0) & (kps0["octave"] <= 1))[0]
    assert len(alone) >= 3
    th_feats = [int(alone[0]), int(alone[1])]
    only_feat = int(alone[2])  # three points on one isolated feature: the second and third find their only candidate taken
    picks = rng.integers(0, len(kps0), N_LIST[0])
    pts0, pick0 = make_points(rng, kfs[0], N_LIST[0], S[0], picks=picks,
                              thresholds=((3, th_feats[0], 50), (4, th_feats[1], 51), (10, only_feat, 5), (11, only_feat, 6), (12, only_feat, 7)))
    pts1, pick1 = make_points(rng, kfs[1], N_LIST[1], S[1])
    points = np.concatenate([pts0, pts1])
    first, count = np.array([0, N_LIST[0]], np.int32), np.array(N_LIST, np.int32)
    # vpMatched on entry: features of keyframe 2 (indices into its feature list), or a point that is in neither keyframe
    n2 = 280  # keyframe 2's features
    rows = []
    for f, share in ((0, 0.12), (1, 0.02)):
        n = len(kfs[f][0])
        row = np.full(n, -1, np.int32)
        occ = rng.random(n) < share
        row[occ] = np.where(rng.random(int(occ.sum())) < 0.8, rng.integers(0, n2, int(occ.sum())), MATCHED_ELSEWHERE)
        rows.append(row)
    for f in th_feats + [only_feat]:
        rows[0][f] = -1
    # keyframe-2 feature -> the point of the list it holds (mvpLoopMapPoints is gathered from keyframe 2's neighbourhood)
    maps = []
    for q_ in range(2):
        pf2 = np.full(n2, -1, np.int32)
        named = rows[q_][rows[q_] >= 0]
        some = named[rng.random(len(named)) < 0.6]
        pf2[some] = rng.integers(13, N_LIST[q_], len(some))
        maps.append(pf2)
    found = (rng.random(len(points)) < 0.04).astype(np.uint8)
    found[[3, 4, 10, 11, 12]] = 0
    queries = np.array([query(0, S[0], found_from_match=1), query(1, S[1])], QUERY)
    cap = max(len(k) for k, _ in kfs) + 13
    return dict(kfs=kfs, points=points, first=first, count=count, rows=rows, maps=maps, found=found, queries=queries, capacity=cap, n2=n2,
                sf=SCALE, bounds=BOUNDS, picks=(pick0, pick1), th_points=(3, 4), only_points=(10, 11, 12))


def restate(sc, k, **kw):
    """query k of a scene through search()"""
    q = sc["queries"][k]
    kps, desc = sc["kfs"][int(q["frame"])]
    a, c = int(sc["first"][k]), int(sc["count"][k])
    found = None if sc.get("found") is None else sc["found"][a:a + c]
    return search(kps, desc, sc["points"][a:a + c], q, sc["rows"][k], found, sc["maps"][k], sc["sf"], sc["bounds"], **kw)


_shared = None


def shared():
    """(the scene, the restatement's result per query), computed once"""
    global _shared
    if _shared is None:
        sc = scene()
        _shared = (sc, [restate(sc, k) for k in range(len(sc["queries"]))])
    return _shared


# ---------------------------------------------------------------------------------------------------------------- the greedy hand case

def hand_greedy():
    """Two level-0 features A (index 0) and B (index 1) four pixels apart and three points that all see both: point 0 is nearest A (distance
    3 to A, 20 to B), point 1 is nearest A too (5 to A, 9 to B), point 2 is nearest B (30 to A, 12 to B).  In list order point 0 takes A,
    point 1 finds A taken and takes B, point 2 finds both taken: no match.  Had point 1 not taken B, point 2 would have: the third point's
    answer depends on the first two accepts.
    -> dict(kps, desc, points, query, expected loop_match)"""
    rng = np.random.default_rng(77)
    kps = np.zeros(2, lr.hb.KP)
    kps["x"], kps["y"], kps["octave"], kps["size"] = [248.0, 252.0], [240.0, 240.0], 0, 31
    A = rng.integers(0, 256, 32, dtype=np.uint8)
    B = A.copy()
    B[:4] ^= 0xFF  # 32 bits apart, in bytes 0 .. 3
    desc = np.stack([A, B])

    def between(da, db):
        """a descriptor `da` bits from A and `db` from B: x bits of bytes 0 .. 3 taken from B, y bits flipped elsewhere"""
        x, y = (da - db + 32) // 2, (da + db - 32) // 2
        assert x >= 0 and y >= 0 and x + y == da and (32 - x) + y == db
        d = np.unpackbits(A)
        bb = np.unpackbits(B)
        d[:x] = bb[:x]
        d[40:40 + y] ^= 1
        return np.packbits(d)
    S = np.eye(4, dtype=f32)
    S[:3, :] *= f32(2.0)  # scale 2: Rcw = I, tcw = 0 once unscaled
    pts = np.zeros(3, MAP_POINT)
    for i, (da, db) in enumerate(((3, 29), (5, 29), (30, 12))):
        pts["pos"][i] = [0.0, 0.0, 2.0]  # u = 250, v = 240: both features two pixels away
        pts["normal"][i], pts["min_distance"][i], pts["max_distance"][i] = (0, 0, 1), 0.5, 1.9  # 1.9 / 2.0 <= 1: level 0
        pts["desc"][i] = between(da, db)
    return dict(kps=kps, desc=desc, points=pts, query=query(0, S), expected=np.array([0, 1], np.int32))
