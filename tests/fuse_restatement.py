"""ORBmatcher::Fuse without its write-back, restated point by point in plain Python / numpy for the tests, as include/amos_frontend.h ("fuse
search") defines the arithmetic -- float32 operation by operation, float64 where OpenCV's gemm, cv::norm and Mat::dot use it: the pre-filter
of ORBmatcher.cc:1042-1083 (Fuse(pKF, Scw, ...): :1199-1244), KeyFrame::GetFeaturesInArea (KeyFrame.cc:752-797) over a grid built as
Frame::AssignFeaturesToGrid builds it, and the candidate loop of :1086-1148 (:1251-1289).  Also the seeded scene the CPU and GPU tests share."""
import types

import numpy as np

import local_points_restatement as lr

f32, f64 = np.float32, np.float64
LOCAL, SIM3 = 0, 1
COLS, ROWS = 64, 48
MAP_POINT = lr.MAP_POINT
CAMERA = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                   ("mbf", "<f4"), ("th", "<f4")])
WINDOW_QUERY = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("level", "<i4"), ("src", "<i4"), ("desc", "u1", (32,))])
REASONS = {"skip": 1, "behind": 2, "image": 3, "near": 4, "far": 5, "angle": 6}
SCALE = lr.HAND_SCALE
INV_SIGMA2 = (f32(1.0) / (SCALE * SCALE)).astype(f32)  # ORBextractor.cc:516-533: mvInvLevelSigma2 = 1.0f / (scale * scale)
BOUNDS = (-70.0, 570.0, 0.0, 480.0)  # 640 x 480 with a negative mnMinX: a cell is 10 x 10 pixels


def prefilter(points, skip, cam, scale_factors, bounds, mode):
    """-> (WINDOW_QUERY per point: u, v, ur, level where in view and zeros elsewhere, src = i, the descriptor; in_view u8; reason)"""
    points = np.ascontiguousarray(points, MAP_POINT)
    sf = np.asarray(scale_factors, f32)
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    n = len(points)
    q = np.zeros(n, WINDOW_QUERY)
    q["src"], q["desc"] = np.arange(n), points["desc"]
    in_view, reason = np.zeros(n, np.uint8), np.zeros(n, np.int8)
    R, t, Ow = cam["Rcw"].astype(f64).reshape(3, 3), cam["tcw"].astype(f64), cam["Ow"].astype(f32)
    fx, fy, cx, cy, mbf = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy", "mbf"))
    with np.errstate(all="ignore"):
        for i in range(n):
            if (points["flags"][i] & lr.SKIP) or (skip is not None and skip[i]):  # :1042-1047 (:1208-1210)
                reason[i] = REASONS["skip"]
                continue
            P = points["pos"][i].astype(f32)
            Pd = P.astype(f64)
            Pc = [f32(((R[r, 0] * Pd[0] + R[r, 1] * Pd[1]) + R[r, 2] * Pd[2]) + t[r]) for r in range(3)]  # :1049-1050
            if Pc[2] < f32(0):                                                                            # :1053-1054
                reason[i] = REASONS["behind"]
                continue
            invz = f32(1) / Pc[2]                                                                         # :1056
            x, y = f32(Pc[0] * invz), f32(Pc[1] * invz)
            u, v = f32(f32(fx * x) + cx), f32(f32(fy * y) + cy)                                           # :1060-1061
            if not (u >= min_x and u < max_x and v >= min_y and v < max_y):                               # KeyFrame::IsInImage
                reason[i] = REASONS["image"]
                continue
            PO = (P - Ow).astype(f32)
            POd = PO.astype(f64)
            dist = f32(np.sqrt((POd[0] * POd[0] + POd[1] * POd[1]) + POd[2] * POd[2]))                    # :1069-1070
            lo, hi = f32(f32(0.8) * points["min_distance"][i]), f32(f32(1.2) * points["max_distance"][i])
            if dist < lo or dist > hi:                                                                    # :1073-1074
                reason[i] = REASONS["near"] if dist < lo else REASONS["far"]
                continue
            Pn = points["normal"][i].astype(f64)
            if ((POd[0] * Pn[0] + POd[1] * Pn[1]) + POd[2] * Pn[2]) < 0.5 * f64(dist):                    # :1079-1080
                reason[i] = REASONS["angle"]
                continue
            q["u"][i], q["v"][i] = u, v
            q["ur"][i] = f32(u - f32(mbf * invz)) if mode == LOCAL else 0                                 # :1064
            q["level"][i] = lr.table_level(f32(points["max_distance"][i]) / dist, sf)                      # :1083
            in_view[i] = 1
    return q, in_view, reason


class Grid:
    """mGrid[x][y] of one keyframe: feature indices in insertion order (Frame::AssignFeaturesToGrid with PosInGrid)"""

    def __init__(self, kps, bounds):
        self.cells = {}
        for i, c in enumerate(lr.grid_cells(kps, bounds)):
            if c >= 0:
                self.cells.setdefault(int(c), []).append(i)
        self.min_x, self.min_y = f32(bounds[0]), f32(bounds[2])
        self.winv, self.hinv = f32(COLS) / f32(f32(bounds[1]) - f32(bounds[0])), f32(ROWS) / f32(f32(bounds[3]) - f32(bounds[2]))

    def area(self, kps, x, y, r):
        """KeyFrame::GetFeaturesInArea -> [(feature, cell)] in the reference's visiting order"""
        x, y, r = f32(x), f32(y), f32(r)
        x0 = max(0, int(np.floor(f32(f32(f32(x - self.min_x) - r) * self.winv))))
        if x0 >= COLS:
            return []
        x1 = min(COLS - 1, int(np.ceil(f32(f32(f32(x - self.min_x) + r) * self.winv))))
        if x1 < 0:
            return []
        y0 = max(0, int(np.floor(f32(f32(f32(y - self.min_y) - r) * self.hinv))))
        if y0 >= ROWS:
            return []
        y1 = min(ROWS - 1, int(np.ceil(f32(f32(f32(y - self.min_y) + r) * self.hinv))))
        if y1 < 0:
            return []
        out = []
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for idx in self.cells.get(ix * ROWS + iy, ()):
                    if abs(f32(kps["x"][idx] - x)) < r and abs(f32(kps["y"][idx] - y)) < r:
                        out.append((idx, ix * ROWS + iy))
        return out


def search_point(grid, kps, bits, u_right, q, th, scale_factors, inv_sigma2, mode, max_dist, info=None):
    """The search of ONE point in view -> (best_idx or -1, best_dist or 256).  info (a dict) collects what the tests' conditions count."""
    sf = np.asarray(scale_factors, f32)
    level = int(q["level"])
    u, v, ur = f32(q["u"]), f32(q["v"]), f32(q["ur"])
    cand = grid.area(kps, u, v, f32(f32(th) * sf[level]))                                                # :1086-1088
    qbits = np.unpackbits(q["desc"])
    best_dist, best_idx, best_cell = 256, -1, -1
    cells_at_best = set()
    lost = {}  # chi-square constant -> the nearest distance it rejected
    if info is not None:
        info["columns"] = len({c // ROWS for _, c in cand})
        info["cells"] = len({c for _, c in cand})
    for idx, cell in cand:
        kp_level = int(kps["octave"][idx])
        if kp_level < level - 1 or kp_level > level:                                                     # :1101-1102
            continue
        dist = int((bits[idx] != qbits).sum())
        if mode == LOCAL:
            ex, ey = f32(u - kps["x"][idx]), f32(v - kps["y"][idx])
            e2 = f32(f32(ex * ex) + f32(ey * ey))
            if u_right is not None and u_right[idx] >= 0:                                                # :1104-1118
                er = f32(ur - f32(u_right[idx]))
                e2 = f32(e2 + f32(er * er))
                if f64(f32(e2 * f32(inv_sigma2[kp_level]))) > 7.8:
                    lost[7.8] = min(lost.get(7.8, 256), dist)
                    continue
            elif f64(f32(e2 * f32(inv_sigma2[kp_level]))) > 5.99:                                        # :1119-1131
                lost[5.99] = min(lost.get(5.99, 256), dist)
                continue
        if dist < best_dist:                                                                             # :1137-1141
            best_dist, best_idx, best_cell = dist, idx, cell
            cells_at_best = {cell}
        elif dist == best_dist:
            cells_at_best.add(cell)
    if info is not None:
        info["tie"] = best_dist <= max_dist and len(cells_at_best) > 1
        info["chi_lost"] = [k for k, d in lost.items() if d < best_dist and d <= max_dist]
    return (best_idx if best_dist <= max_dist else -1), best_dist                                        # :1146


def fuse(kfs, points, pairs, skip, n_out, scale_factors, inv_sigma2, bounds, mode, max_dist=50, with_right=True, infos=None):
    """kfs: [(kps, desc, u_right)]; pairs: [(frame, first, count, out_off, camera)]; skip: u8 [n_out] or None.
    -> dict(query, in_view, best_idx, best_dist [n_out], stats [pairs][2], reason [n_out])"""
    query, in_view = np.zeros(n_out, WINDOW_QUERY), np.zeros(n_out, np.uint8)
    best_idx, best_dist = np.full(n_out, -1, np.int32), np.full(n_out, 256, np.int32)
    reason, stats = np.zeros(n_out, np.int8), np.zeros((len(pairs), 2), np.int32)
    grids = {}
    for p, (frame, first, count, off, cam) in enumerate(pairs):
        kps, desc, ur = kfs[frame]
        if not with_right:
            ur = None
        if frame not in grids:
            grids[frame] = (Grid(kps, bounds), np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1))
        grid, bits = grids[frame]
        sk = None if skip is None else skip[off:off + count]
        q, iv, why = prefilter(points[first:first + count], sk, cam, scale_factors, bounds, mode)
        query[off:off + count], in_view[off:off + count], reason[off:off + count] = q, iv, why
        for i in np.nonzero(iv)[0]:
            info = {} if infos is not None else None
            bi, bd = search_point(grid, kps, bits, ur, q[i], cam["th"], scale_factors, inv_sigma2, mode, max_dist, info)
            best_idx[off + i], best_dist[off + i] = bi, bd
            if infos is not None:
                infos.append((p, int(i), info))
        stats[p] = int(iv.sum()), int((best_idx[off:off + count] >= 0).sum())
    return dict(query=query, in_view=in_view, best_idx=best_idx, best_dist=best_dist, stats=stats, reason=reason)


# ---------------------------------------------------------------------------------------------------------------- the shared scene

def camera(R, t, fx=512.0, fy=512.0, cx=250.0, cy=240.0, mbf=40.0, th=3.0):
    c = np.zeros((), CAMERA)
    c["Rcw"], c["tcw"] = np.asarray(R, f32).reshape(9), np.asarray(t, f32)
    c["Ow"] = (-(np.asarray(R, f32).astype(f64).T @ np.asarray(t, f32).astype(f64))).astype(f32)  # KeyFrame::SetPose: Ow = -Rcw.t() * tcw
    c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], c["th"] = fx, fy, cx, cy, mbf, th
    return c


def flip_bits(rng, desc, k):
    """desc with exactly k of its 256 bits flipped"""
    bits = np.unpackbits(desc)
    bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def make_keyframe(rng, n, twins, stereo_share=0.5):
    """n features: seeded positions, octaves and descriptors, u_right >= 0 on a share of them; the last `twins` features copy an earlier
    feature's descriptor, octave and u_right one cell to the LEFT of it (x - min_x = 14 against 16: cells 1 and 2 of a row), so the copy --
    the higher index -- is the first of the two in the reference's visiting order."""
    kps, desc = np.zeros(n, lr.hb.KP), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if n == 0:
        return kps, desc, np.zeros(0, f32)
    kps["x"] = rng.uniform(BOUNDS[0] + 0.5, BOUNDS[1] - 0.5, n).astype(f32)
    kps["y"] = rng.uniform(BOUNDS[2] + 0.5, BOUNDS[3] - 0.5, n).astype(f32)
    kps["octave"] = rng.integers(0, len(SCALE), n)
    kps["size"], kps["angle"] = 31, rng.uniform(0, 360, n)
    disparity = rng.uniform(3, 30, n)
    ur = np.where(rng.random(n) < stereo_share, kps["x"] - disparity, -1).astype(f32)
    for j in range(twins):
        a, b = j, n - twins + j
        col = 2 + 3 * j
        kps["x"][a], kps["x"][b] = BOUNDS[0] + 10 * col + 6.0, BOUNDS[0] + 10 * col + 4.0
        kps["y"][a] = kps["y"][b] = 100.0 + 7 * j
        kps["octave"][b], desc[b] = kps["octave"][a], desc[a]
        ur[a], ur[b] = kps["x"][a] - 10.0, kps["x"][b] - 10.0
    return kps, desc, ur


def points_of(rng, kf, m, cam, twins=0, thresholds=False, gate_share=0.06, noise=1.1):
    """m points for one keyframe: features back-projected through `cam` at the depth their disparity says (a seeded depth for a monocular
    feature), position noise that puts a share of them beyond either chi-square constant, a few flipped descriptor bits, max_distance for a
    predicted level at the feature's octave or one above; `gate_share` of them fail each pre-filter test.  The first `twins` points sit between
    a twin pair; with `thresholds` the next two have a nearest distance of exactly 50 and 51."""
    kps, desc, ur = kf
    pts = np.zeros(m, MAP_POINT)
    if m == 0:
        return pts
    sf = SCALE.astype(f64)
    n = len(kps)
    pick = rng.integers(twins, max(n - twins, twins + 1), m)
    pick[:twins] = np.arange(twins)
    sd = np.full(m, noise)
    sd[:twins + 2] = 0.05
    k = kps[pick]
    du, dv = rng.normal(0, 1, m) * sd * sf[k["octave"]], rng.normal(0, 1, m) * sd * sf[k["octave"]]
    du[:twins] -= 1.0  # between the pair
    d = np.where(ur[pick] >= 0, k["x"] - ur[pick], rng.uniform(3, 30, m)).astype(f64)
    z = float(cam["mbf"]) / np.maximum(d + np.where(ur[pick] >= 0, rng.normal(0, 1, m) * sd * 0.7 * sf[k["octave"]], 0), 1.0)
    gate = rng.random(m)
    gate[:twins + 2] = 1.0
    g = gate_share
    z = np.where(gate < g, -z, z)
    x = (k["x"].astype(f64) + du - float(cam["cx"])) / float(cam["fx"]) * z
    y = (k["y"].astype(f64) + dv - float(cam["cy"])) / float(cam["fy"]) * z
    x = np.where((gate >= g) & (gate < 2 * g), x + 3.0 * z, x)
    R, t = cam["Rcw"].astype(f64).reshape(3, 3), cam["tcw"].astype(f64)
    pts["pos"] = ((np.stack([x, y, z], 1) - t) @ R).astype(f32)
    PO = pts["pos"].astype(f64) - cam["Ow"].astype(f64)
    dist = np.linalg.norm(PO, axis=1)
    toward = PO / dist[:, None]
    side = np.cross(toward, rng.normal(0, 1, (m, 3)))
    side /= np.linalg.norm(side, axis=1)[:, None]
    away = (gate >= 2 * g) & (gate < 3 * g)
    normal = np.where(away[:, None], 0.2 * toward + side, toward + rng.normal(0, 0.15, (m, 3)))
    pts["normal"] = (normal / np.linalg.norm(normal, axis=1)[:, None]).astype(f32)
    level = np.minimum(k["octave"] + rng.integers(0, 2, m), len(sf) - 1)
    pts["max_distance"] = (dist * sf[level] * rng.uniform(0.93, 0.99, m)).astype(f32)
    pts["min_distance"] = (pts["max_distance"] / sf[-1] / 1.5).astype(f32)
    far, near = (gate >= 3 * g) & (gate < 4 * g), (gate >= 4 * g) & (gate < 5 * g)
    pts["max_distance"] = np.where(far, dist / 1.3, np.where(near, dist * 3, pts["max_distance"])).astype(f32)
    pts["min_distance"] = np.where(near, dist * 1.4, np.where(far, dist / 10, pts["min_distance"])).astype(f32)
    pts["flags"] = np.where((gate >= 5 * g) & (gate < 6 * g), lr.SKIP, 0)
    for i in range(m):
        pts["desc"][i] = flip_bits(rng, desc[pick[i]], int(rng.integers(0, 12)))
    if thresholds:
        pts["desc"][twins], pts["desc"][twins + 1] = flip_bits(rng, desc[pick[twins]], 50), flip_bits(rng, desc[pick[twins + 1]], 51)
    return pts


def hand_points(rng):
    """One point per pre-filter outcome for the camera camera(I, 0) (fx = 512, cx = 250: u = 512 x + 250 is exact for x = +-0.625):
    -> (points, expected reason per point; 0 = in view)"""
    rows = []

    def add(pos, why, normal=(0, 0, 1), min_d=0.5, max_d=4.7):
        p = np.zeros((), MAP_POINT)
        p["pos"], p["normal"], p["min_distance"], p["max_distance"] = pos, normal, min_d, max_d
        p["desc"] = rng.integers(0, 256, 32, dtype=np.uint8)
        rows.append((p, why))
    add((0.1, 0.1, -1.0), "behind")
    add((0.3, 0.2, 0.0), "image")                       # z == 0: the projection is infinite
    add((0.0, 0.0, 0.0), "image")                       # 0 * inf
    add((np.nan, 0.1, 2.0), "image")
    add((0.1, np.nan, 2.0), "image")
    add((0.1, 0.1, np.nan), "image")
    add((0.625 * 2, 0.0, 2.0), "image")                 # u == max_x exactly: out
    add((-0.625 * 2, 0.0, 2.0), 0)                      # u == min_x exactly: in
    add((0.0, 0.46875 * 2, 2.0), "image")               # v == max_y exactly (512 * 0.46875 + 240 = 480)
    add((0.0, -0.46875 * 2, 2.0), 0)                    # v == min_y exactly
    lo, hi = f32(f32(0.8) * f32(2.3)), f32(f32(1.2) * f32(1.9))
    add((0.0, 0.0, lo), 0, min_d=2.3, max_d=4.1)        # dist3D == 0.8f * min_distance: in
    add((0.0, 0.0, np.nextafter(lo, f32(0))), "near", min_d=2.3, max_d=4.1)
    add((0.0, 0.0, hi), 0, min_d=0.5, max_d=1.9)        # dist3D == 1.2f * max_distance: in
    add((0.0, 0.0, np.nextafter(hi, f32(9))), "far", min_d=0.5, max_d=1.9)
    add((0.0, 0.0, 2.0), 0, normal=(0.8, 0.0, 0.5))     # PO . Pn == 0.5 * dist3D: in
    add((0.0, 0.0, 2.0), "angle", normal=(0.8, 0.0, np.nextafter(f32(0.5), f32(0))))
    p = np.zeros((), MAP_POINT)
    p["pos"], p["normal"], p["min_distance"], p["max_distance"], p["flags"] = (0, 0, 2), (0, 0, 1), 0.5, 4.7, lr.SKIP
    rows.append((p, "skip"))
    pts = np.array([r[0] for r in rows], MAP_POINT)
    return pts, np.array([REASONS[w] if w else 0 for _, w in rows], np.int8)


def scene(seed=11):
    """4 keyframes of 0 / 37 / 300 / 600 features and 7 pairs: the point counts 0, 1, 31, 33, 257 and 700, and a seventh pair that shares the
    257-point range with pair 4 under another camera and other skip bytes.  Pair 5 (700 points, keyframe 3) starts with the hand points, the
    tie points and the two threshold points; pair 3 has th = 40: windows wider than 8 grid columns; pair 1 is on the empty keyframe."""
    rng = np.random.default_rng(seed)
    twins = 6
    kfs = [make_keyframe(rng, 0, 0), make_keyframe(rng, 37, 0), make_keyframe(rng, 300, 0), make_keyframe(rng, 600, twins)]
    eye = np.eye(3, dtype=f32)
    cams = [camera(*lr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1])),              # 0 points
            camera(eye, [0, 0, 0]),                                                # 1 point on the empty keyframe
            camera(*lr.pose(-0.015, 0.01, -0.01, [-0.03, 0.04, -0.05])),           # 31
            camera(*lr.pose(0.02, 0.01, 0.0, [0.02, 0.0, 0.03]), th=40.0),         # 33
            camera(*lr.pose(0.0, -0.01, 0.02, [0.0, 0.05, -0.02]), th=3.0),        # 257
            camera(eye, [0, 0, 0], th=3.0),                                        # 700
            camera(*lr.pose(0.0, -0.01, 0.02, [0.0005, 0.05, -0.02]), th=5.0)]     # the 257 again
    hand, hand_reason = hand_points(rng)
    lists = [points_of(rng, kfs[1], 0, cams[0]), points_of(rng, kfs[1], 1, cams[1]), points_of(rng, kfs[1], 31, cams[2], gate_share=0.03),
             points_of(rng, kfs[1], 33, cams[3], gate_share=0.03), points_of(rng, kfs[2], 257, cams[4]),
             np.concatenate([hand, points_of(rng, kfs[3], 700 - len(hand), cams[5], twins=twins, thresholds=True)])]
    first = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int32)
    points = np.concatenate(lists)
    frames = [1, 0, 1, 1, 2, 3, 2]
    firsts = [int(first[k]) for k in range(6)] + [int(first[4])]
    counts = [len(p) for p in lists] + [257]
    offs, o = [], 3  # a gap in front of the first pair and between pairs: entries no pair owns
    for c in counts:
        offs.append(o)
        o += c + 2
    n_out = o
    skip = (rng.random(n_out) < 0.05).astype(np.uint8)
    skip[offs[5]:offs[5] + len(hand) + twins + 2] = 0
    skip[offs[1]] = 0  # the point on the empty keyframe is in view: its window is searched, and holds nothing
    pairs = [(frames[p], firsts[p], counts[p], offs[p], cams[p]) for p in range(7)]
    return dict(kfs=kfs, points=points, pairs=pairs, skip=skip, n_out=n_out, hand=(offs[5], hand_reason), twins=(offs[5] + len(hand), twins),
                sf=SCALE, inv_sigma2=INV_SIGMA2, bounds=BOUNDS)


def oracle_pair(ob_hb, kf, points, skip, cam, scale_factors, inv_sigma2, bounds, mode, with_right=True):
    """The same pair through tests/adaptor_prefilter.py keyframe_queries (level in the table form) and the oracle's orc_window_search
    -> (best_idx per point, accepted count)"""
    import adaptor_prefilter as ap
    kps, desc, ur = kf
    n = len(points)
    best = np.full(n, -1, np.int32)
    if len(kps) == 0 or n == 0:
        return best, 0
    shim = types.SimpleNamespace(WINDOW_QUERY=ob_hb.WINDOW_QUERY,
                                 standin_predict_scale=lambda md, cd, _sf1, _nl: lr.table_level(np.asarray(md, f32) / np.asarray(cd, f32), scale_factors))
    c = types.SimpleNamespace(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], mbf=cam["mbf"], min_x=bounds[0], max_x=bounds[1],
                              min_y=bounds[2], max_y=bounds[3])
    keep = (points["flags"] & lr.SKIP) == 0
    if skip is not None:
        keep &= skip == 0
    with np.errstate(all="ignore"):
        q, pos = ap.keyframe_queries(shim, c, cam["Rcw"].reshape(3, 3), cam["tcw"], cam["Ow"], points["pos"], points["normal"], points["min_distance"],
                                     points["max_distance"], points["desc"], np.arange(n), keep, mode == LOCAL, scale_factors[1], len(scale_factors))
    view, alive = ob_hb.frame_view(kps, desc, ur if with_right else None, tuple(float(b) for b in bounds))
    r, b = ob_hb.fuse("oracle", view, q, scale_factors, float(cam["th"]), inv_sigma2 if mode == LOCAL else None)
    best[pos] = b
    return best, int(r)
