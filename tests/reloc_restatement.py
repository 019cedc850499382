"""Relocalization's ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1731-1863) restated for the
tests in plain numpy / Python exactly as include/amos_frontend.h ("relocalisation search") defines it: the projection and its filters float32
operation by operation (float64 where the definition says so), Frame::GetFeaturesInArea over the 64 x 48 grid, the sequential loop over
the keyframe's points with the features set on entry, the rotation histogram, and every stat.  Also the record builders and seeded scenes
that the CPU and GPU tests share."""
import numpy as np

import host_binding as hb
import local_points_restatement as lr  # grid_cells
import motion_model_restatement as mr  # rotation_bin, three_maxima, pose

POINT = np.dtype([("pos", "<f4", (3,)), ("angle", "<f4"), ("min_distance", "<f4"), ("max_distance", "<f4"), ("flags", "<i4"),
                  ("desc", "u1", (32,)), ("pad", "u1", (4,))])
CAMERA = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("th", "<f4"),
                   ("orb_dist", "<i4"), ("check_orientation", "<i4"), ("found_from_match", "<i4"), ("enabled", "<i4")])
SKIP, HAS_OBS = 1, 2
HISTO_LENGTH = 30
STAT_FIELDS = ("n_candidates", "n_projected", "n_matches", "n_researched", "n_found", "n_occupied", "status", "skipped")
f32, f64 = np.float32, np.float64


def camera(Rcw, tcw, fx, fy, cx, cy, th=10.0, orb_dist=100, check_orientation=1, found_from_match=0, enabled=1):
    c = np.zeros((), CAMERA)
    c["Rcw"], c["tcw"] = np.asarray(Rcw, f32).reshape(9), tcw
    c["fx"], c["fy"], c["cx"], c["cy"], c["th"] = fx, fy, cx, cy, th
    c["orb_dist"], c["check_orientation"], c["found_from_match"], c["enabled"] = orb_dist, check_orientation, found_from_match, enabled
    return c


def camera_centre(Rcw, tcw):
    """Ow = -Rcw^T tcw: one gemm per row in double, one rounding (as amos_pose_result.Ow)."""
    R, t = np.asarray(Rcw, f32).astype(f64).reshape(3, 3), np.asarray(tcw, f32).astype(f64)
    return np.array([f32(-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2])) for k in range(3)], f32)


def predict_level(max_distance, dist, scale_factors):
    """The table-count form of MapPoint::PredictScale: the ratio is mfMaxDistance / dist (MapPoint.cc:576)."""
    with np.errstate(all="ignore"):
        ratio = f32(max_distance) / f32(dist)
    sf = np.asarray(scale_factors, f32)
    return min(int((ratio > sf).sum()), len(sf) - 1)


def found_of(points, cam, found, match_in):
    """sAlreadyFound as one byte per point: the caller's array, and with found_from_match the points that the entry matches name."""
    fd = np.zeros(len(points), bool) if found is None else np.asarray(found) != 0
    if int(cam["found_from_match"]):
        m = np.asarray(match_in)
        m = m[(m >= 0) & (m < len(points))]
        fd = fd.copy()
        fd[m] = True
    return fd


def project(points, cam, found, scale_factors, bounds, pose=None):
    """-> (query records [hb.KF_QUERY, every point], projected u8, candidate bool, status).  pose: (Tcw as 12 floats, rows of [R | t];
    Ow) as an amos_pose_result holds them, or None: the camera's pose."""
    points = np.ascontiguousarray(points, POINT)
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    n = len(points)
    q = np.zeros(n, hb.KF_QUERY)
    q["angle"], q["desc"] = points["angle"], points["desc"]
    projected, candidate = np.zeros(n, np.uint8), np.zeros(n, bool)
    status = 0
    if pose is None:
        R, t, Ow = cam["Rcw"].astype(f64).reshape(3, 3), cam["tcw"].astype(f64), camera_centre(cam["Rcw"], cam["tcw"])
    else:
        T = np.asarray(pose[0], f32).reshape(3, 4).astype(f64)
        R, t, Ow = T[:, :3], T[:, 3], np.asarray(pose[1], f32)
    fx, fy, cx, cy = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        for i in range(n):
            if (points["flags"][i] & SKIP) or found[i]:
                continue
            candidate[i] = True
            Pf = points["pos"][i]
            P = Pf.astype(f64)
            xc, yc, zc = (f32(((R[r, 0] * P[0] + R[r, 1] * P[1]) + R[r, 2] * P[2]) + t[r]) for r in range(3))
            invz = f32(f64(1.0) / f64(zc))  # no sign test
            u = f32(f32(fx * xc) * invz) + cx
            v = f32(f32(fy * yc) * invz) + cy
            if not (np.isfinite(u) and np.isfinite(v)):
                status |= 1
                continue
            if u < min_x or u > max_x or v < min_y or v > max_y:
                continue
            PO = (Pf - Ow).astype(f64)
            dist = f32(np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]))
            if dist < f32(0.8) * points["min_distance"][i] or dist > f32(1.2) * points["max_distance"][i]:
                continue
            q["u"][i], q["v"][i] = u, v
            q["level"][i] = predict_level(points["max_distance"][i], dist, scale_factors)
            projected[i] = 1
    return q, projected, candidate, status


class Grid:
    """Frame::GetFeaturesInArea (Frame.cc:894-1003) over Frame::PosInGrid's cells: the candidates of a window in the reference's order
    (cells x-major, then y, then insertion order = feature index)."""

    def __init__(self, kps, bounds):
        self.x, self.y, self.octave = kps["x"].astype(f32), kps["y"].astype(f32), kps["octave"].astype(np.int64)
        self.min_x, self.max_x, self.min_y, self.max_y = (f32(b) for b in bounds)
        self.winv, self.hinv = f32(64) / f32(self.max_x - self.min_x), f32(48) / f32(self.max_y - self.min_y)
        self.cell = lr.grid_cells(kps, bounds).astype(np.int64)
        self.order = np.lexsort((np.arange(len(kps)), self.cell))

    def area(self, u, v, r, lo, hi):
        u, v, r = f32(u), f32(v), f32(r)
        x0 = int(np.floor(f32(f32(f32(u - self.min_x) - r) * self.winv)))
        x1 = int(np.ceil(f32(f32(f32(u - self.min_x) + r) * self.winv)))
        y0 = int(np.floor(f32(f32(f32(v - self.min_y) - r) * self.hinv)))
        y1 = int(np.ceil(f32(f32(f32(v - self.min_y) + r) * self.hinv)))
        x0, y0 = max(x0, 0), max(y0, 0)
        x1, y1 = min(x1, 63), min(y1, 47)
        if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
            return np.zeros(0, np.int64)
        cx, cy = self.cell // 48, self.cell % 48
        ok = (self.cell >= 0) & (cx >= x0) & (cx <= x1) & (cy >= y0) & (cy <= y1) & (self.octave >= lo) & (self.octave <= hi)
        ok &= (np.abs(self.x - u) < r) & (np.abs(self.y - v) < r)
        return self.order[ok[self.order]]


def search(kps, desc, points, cam, found, match_in, scale_factors, bounds, pose=None):
    """One pair.  match_in [len(kps)]: the frame's matches on entry (index into `points`, or -1).  -> dict(query, projected, match, and
    every field of amos_reloc_stats)."""
    points = np.ascontiguousarray(points, POINT)
    match = np.asarray(match_in, np.int32).copy()
    n = len(kps)
    assert len(match) == n
    if not int(cam["enabled"]):
        out = dict(query=np.zeros(len(points), hb.KF_QUERY), projected=np.zeros(len(points), np.uint8), match=match)
        out.update({k: 0 for k in STAT_FIELDS}, skipped=1)
        return out
    fd = found_of(points, cam, found, match)
    q, projected, candidate, status = project(points, cam, fd, scale_factors, bounds, pose)
    sf = np.asarray(scale_factors, f32)
    th, orb_dist, check_ori = f32(cam["th"]), int(cam["orb_dist"]), bool(cam["check_orientation"])
    grid = Grid(kps, bounds)
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.int16)
    on_entry = match >= 0
    entries = []  # one (feature, bin) per accepted point
    n_matches = n_researched = 0
    for i in np.nonzero(projected)[0]:
        level = int(q["level"][i])
        cand = grid.area(q["u"][i], q["v"][i], th * sf[level], level - 1, level + 1)
        if len(cand) == 0:
            continue
        d = np.abs(bits[cand] - np.unpackbits(q["desc"][i]).astype(np.int16)[None, :]).sum(1)
        free_on_entry = [(int(d[k]), k) for k in range(len(cand)) if not on_entry[cand[k]] and d[k] < 256]
        if len(free_on_entry) >= 2:
            two = sorted(free_on_entry)[:2]
            n_researched += bool(match[cand[two[0][1]]] >= 0 and match[cand[two[1][1]]] >= 0)
        best_dist, best = 256, -1
        for k in range(len(cand)):
            if match[cand[k]] >= 0:
                continue
            if d[k] < best_dist:
                best_dist, best = int(d[k]), int(cand[k])
        if best_dist <= orb_dist:
            match[best] = i
            n_matches += 1
            if check_ori:
                entries.append((best, mr.rotation_bin(q["angle"][i], kps["angle"][best])))
    if check_ori:
        winners = mr.three_maxima(np.bincount([b for _, b in entries], minlength=HISTO_LENGTH))
        for i2, b in entries:
            if b not in winners:
                match[i2] = -1
                n_matches -= 1
    skipped = (points["flags"] & SKIP) != 0
    return dict(query=q, projected=projected, match=match, n_candidates=int(candidate.sum()), n_projected=int(projected.sum()),
                n_matches=n_matches, n_researched=n_researched, n_found=int((fd & ~skipped).sum()), n_occupied=int(on_entry.sum()),
                status=status, skipped=0)


# ---------------------------------------------------------------------------------------------------------------- record builders

def distances(pos, kf_pose, kf_levels, scale_factors):
    """mfMinDistance / mfMaxDistance as MapPoint::UpdateNormalAndDepth sets them from the reference keyframe: max = dist * scale[level of the
    keypoint], min = max / scale[n_levels - 1]."""
    sf = np.asarray(scale_factors, f32)
    Ow = camera_centre(kf_pose[0], kf_pose[1])
    PO = (np.asarray(pos, f32) - Ow[None, :]).astype(f64)
    dist = np.sqrt((PO[:, 0] ** 2 + PO[:, 1] ** 2) + PO[:, 2] ** 2).astype(f32)
    mx = (dist * sf[np.asarray(kf_levels)]).astype(f32)
    return (mx / sf[-1]).astype(f32), mx


def make_points(rng, kf_kps, kf_desc, m, kf_pose, intr, scale_factors, skip_share=0.1, replace=False, behind=True):
    """m keyframe features with their map points: keypoints of the keyframe (in order, or drawn with replacement: several points then contend
    for one feature of the current frame), back-projected at seeded depths through the keyframe's pose.  About 70 % have observations,
    `skip_share` carry the skip flag, a few descriptor bits are flipped, and point 0 (when there are more than one) lies behind the camera."""
    pts = np.zeros(m, POINT)
    if m == 0:
        return pts
    fx, fy, cx, cy = intr
    pick = rng.integers(0, len(kf_kps), m) if replace else np.arange(m) % len(kf_kps)
    k = kf_kps[pick]
    z = rng.uniform(2.0, 6.0, m)
    if m > 1 and behind:
        z[0] = -z[0]
    x = (k["x"].astype(f64) + rng.normal(0, 0.5, m) - cx) / fx * z
    y = (k["y"].astype(f64) + rng.normal(0, 0.5, m) - cy) / fy * z
    R, t = kf_pose[0].astype(f64), kf_pose[1].astype(f64)
    pts["pos"] = ((np.stack([x, y, z], 1) - t) @ R).astype(f32)  # R^T (Pk - t)
    pts["angle"] = k["angle"]
    pts["min_distance"], pts["max_distance"] = distances(pts["pos"], kf_pose, k["octave"], scale_factors)
    pts["flags"] = np.where(rng.random(m) < 0.7, HAS_OBS, 0) | np.where(rng.random(m) < skip_share, SKIP, 0)
    pts["desc"] = kf_desc[pick]
    flip = rng.random((m, 32)) < 0.02
    pts["desc"] ^= (flip * (1 << rng.integers(0, 8, (m, 32)))).astype(np.uint8)
    return pts


def entry_state(rng, n_features, n_points, occupied_share=1.0 / 3, found_share=0.2):
    """(match_in, found): a third of the features set on entry (each names a seeded point), a fifth of the points found."""
    match = np.full(n_features, -1, np.int32)
    if n_points > 0 and n_features > 0:
        occ = rng.random(n_features) < occupied_share
        match[occ] = rng.integers(0, n_points, int(occ.sum()))
    found = (rng.random(n_points) < found_share).astype(np.uint8)
    return match, found


KF_POSE = mr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1])
CUR_MOTIONS = [dict(t=(0.015, -0.01, 0.005), ry=0.002), dict(t=(-0.01, 0.008, -0.02), rx=-0.0015, rz=0.001)]
PARAMS = [(10.0, 100), (3.0, 64)]  # (th, ORBdist) of Tracking.cc:2732 and :2756


# ---------------------------------------------------------------------------------------------------------------- hand cases

HAND_BOUNDS = mr.HAND_BOUNDS
HAND_SCALE = mr.HAND_SCALE
HAND_INTR = (512.0, 512.0, 320.0, 240.0)
EYE, ZERO = np.eye(3, dtype=f32), np.zeros(3, f32)


def hand_camera(**kw):
    return camera(EYE, ZERO, *HAND_INTR, **kw)


def hand_point(kps, desc, feature, angle=0.0, du=0.0, flip_bits=0, z=1.0, flags=HAS_OBS, dist_range=(0.5, 2.0)):
    """One point that an identity pose projects onto `feature` (+ du in x) from depth z, with the feature's descriptor (the first `flip_bits`
    bits flipped).  With min = 0.5 and max = 2.0 a point at distance ~1 predicts level 4 of HAND_SCALE (2.0 > 1, 1.2, 1.44, 1.728), so the
    hand frames put their features on level 4 and a radius of th = 3 is 3 * 2.0736 = 6.2 px."""
    p = np.zeros(1, POINT)
    p["pos"] = [f64(kps["x"][feature] + du - 320.0) / 512.0 * z, f64(kps["y"][feature] - 240.0) / 512.0 * z, z]
    p["angle"], p["flags"], p["min_distance"], p["max_distance"] = angle, flags, dist_range[0], dist_range[1]
    d = desc[feature].copy()
    for b in range(flip_bits):
        d[b // 8] ^= 1 << (b % 8)
    p["desc"] = d
    return p


def hand_frame(angles=None):
    kps, desc = mr.hand_frame(angles)
    kps["octave"] = 4
    return kps, desc


# ---------------------------------------------------------------------------------------------------------------- the refinement of one candidate

def refine(kps, desc, kf_points, ident, table_pos, vp_matches, inliers, start, intr, scale_factors, inv_sigma2, bounds):
    """ORB_SLAM2::RefineRelocalization (Tracking.cc:2700-2783 for one candidate) as a chain of restatements.  kf_points: POINT records, one
    per keyframe feature; ident [len(kf_points)]: which MapPoint of the table (`table_pos` [points][3]) sits at the feature, -1 for none;
    vp_matches [len(kps)]: MapPoint of the table or -1; inliers [len(kps)]; start: (Rcw, tcw) of the pose PnP found.
    -> dict(n_good, points [len(kps)] = MapPoint of the table or -1, outlier, Tcw [12], steps: what ran)"""
    import pose_optimization_cases as pc
    import pose_optimization_restatement as pr
    n = len(kps)
    ident = np.asarray(ident)
    mp = np.where(np.asarray(inliers) != 0, np.asarray(vp_matches), -1).astype(np.int32)
    found = set(int(v) for v in np.asarray(vp_matches)[np.asarray(inliers) != 0])
    state = dict(R=np.asarray(start[0], f32).reshape(9), t=np.asarray(start[1], f32), outlier=np.zeros(n, np.uint8))
    steps = []

    def optimise():  # ORB_SLAM2::PoseOptimization: mvbOutlier and SetPose; fewer than 3 edges leave the pose and return 0
        cam = pc.camera(state["R"], state["t"], *intr, 0.0)
        res, out, _ = pr.pose_optimization(kps, None, mp, table_pos, None, cam, inv_sigma2, state["outlier"], 0)
        steps.append("optimise")
        if res["n_edges"] < 3:
            state["outlier"][mp >= 0] = 0
            return 0
        state["outlier"] = out
        T = res["Tcw"].reshape(3, 4)
        state["R"], state["t"] = T[:, :3].reshape(9).copy(), T[:, 3].copy()
        return int(res["n_inliers"])

    def clear():
        mp[state["outlier"] != 0] = -1

    def search_more(th, orb_dist):
        fd = np.array([int(i) >= 0 and int(i) in found for i in ident], np.uint8)
        cam = camera(state["R"], state["t"], *intr, th=th, orb_dist=orb_dist)
        s = search(kps, desc, kf_points, cam, fd, np.where(mp >= 0, 0, -1).astype(np.int32), scale_factors, bounds)
        new = (mp < 0) & (s["match"] >= 0)
        mp[new] = ident[s["match"][new]]
        steps.append("search")
        return s["n_matches"]

    n_good = optimise()
    if n_good >= 10:
        clear()
        if n_good < 50:
            if search_more(10.0, 100) + n_good >= 50:
                n_good = optimise()
                if 30 < n_good < 50:
                    found = set(int(v) for v in mp[mp >= 0])
                    if n_good + search_more(3.0, 64) >= 50:
                        n_good = optimise()
                        clear()
    Tcw = np.concatenate([np.concatenate([state["R"][3 * r:3 * r + 3], state["t"][r:r + 1]]) for r in range(3)]).astype(f32)
    return dict(n_good=n_good, points=mp, outlier=state["outlier"], Tcw=Tcw, steps=steps)


def refine_case(kps, desc, intr, scale_factors, seed, n_inliers, n_usable, n_wrong, n_off=0, shake=1.0):
    """A seeded candidate: the keyframe has the frame's own keypoints (feature i carries MapPoint i, the back-projection of feature i through
    rr.KF_POSE, the true pose), `n_usable` of them with a good point; `n_inliers` of those are PnP inliers on entry, `n_wrong` of these
    matched to another point (an outlier of the first optimisation, whose point is "found" until sFound is rebuilt); `n_off` of the other
    usable points stand about 5 px beside their feature (matched by the first search, outliers of the second optimisation); the start pose
    is the truth moved by `shake` times a fixed small motion.
    -> dict(kf_points, ident, table_pos, vp_matches, inliers, start)"""
    rng = np.random.default_rng(seed)
    n = len(kps)
    pts = make_points(rng, kps, desc, n, KF_POSE, intr, scale_factors, skip_share=0.0, behind=False)
    usable = rng.permutation(n)[:n_usable]
    ident = np.full(n, -1, np.int32)
    ident[usable] = usable
    pts["flags"] = np.where(ident >= 0, pts["flags"] & ~SKIP, SKIP)
    vp = np.full(n, -1, np.int32)
    inl = usable[:n_inliers]
    vp[inl] = inl
    vp[inl[:n_wrong]] = usable[n_inliers:n_inliers + n_wrong]
    extra = usable[n_inliers + n_wrong:n_inliers + n_wrong + 5]  # matches that PnP rejected
    off = usable[n_usable - n_off:] if n_off else usable[:0]
    pts["pos"][off] += (np.array([0.02, -0.012, 0.0]) * 4.0).astype(f32)  # the points lie 2 .. 6 deep: 5 px and more at f = 260
    vp[extra] = extra
    inliers = np.zeros(n, np.uint8)
    inliers[inl] = 1
    start = mr.moved(KF_POSE, rx=0.004 * shake, ry=-0.003 * shake, rz=0.002 * shake, t=(0.01 * shake, -0.008 * shake, 0.006 * shake))
    return dict(kf_points=pts, ident=ident, table_pos=pts["pos"].copy(), vp_matches=vp, inliers=inliers, start=start)
