"""The search of Tracking::TrackWithMotionModel (Tracking.cc:1925-1945) restated for the tests: the projection of the last frame's points and
the forward / backward flags in numpy exactly as include/amos_frontend.h ("motion-model search") defines their arithmetic -- float32
operation by operation, float64 where the definition says so --, then ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) by
the CPU oracle (orc_search_by_projection_frame) on the projected records, and the second search below retry_below matches.  Also a
pure-Python restatement of the greedy loop with its rotation histogram (the hand cases compare it with the oracle), and the seeded scenes
the CPU and GPU tests share."""
import ctypes as C
import math

import numpy as np

import host_binding as hb
import oracle_binding as ob

LAST_POINT = np.dtype([("pos", "<f4", (3,)), ("angle", "<f4"), ("octave", "<i4"), ("flags", "<i4"), ("desc", "u1", (32,)), ("pad", "u1", (8,))])
CAMERA = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Rlw", "<f4", (9,)), ("tlw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"),
                   ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4"), ("mb", "<f4"), ("th", "<f4"), ("th_retry", "<f4"), ("retry_below", "<i4"),
                   ("mono", "<i4"), ("check_orientation", "<i4")])
SKIP, HAS_OBS = 1, 2
FORWARD, BACKWARD = 1, 2
TH_HIGH, HISTO_LENGTH = 100, 30
f32, f64 = np.float32, np.float64


def camera(Rcw, tcw, Rlw, tlw, fx, fy, cx, cy, mb=0.02, th=15.0, th_retry=None, retry_below=20, mono=0, check_orientation=1):
    c = np.zeros((), CAMERA)
    c["Rcw"], c["tcw"], c["Rlw"], c["tlw"] = np.asarray(Rcw, f32).reshape(9), tcw, np.asarray(Rlw, f32).reshape(9), tlw
    c["fx"], c["fy"], c["cx"], c["cy"], c["mb"] = fx, fy, cx, cy, mb
    c["mbf"] = f32(mb) * f32(fx)
    c["th"], c["th_retry"] = th, 2 * th if th_retry is None else th_retry
    c["retry_below"], c["mono"], c["check_orientation"] = retry_below, mono, check_orientation
    return c


def motion_flags(cam):
    """bForward / bBackward of ORBmatcher.cc:1584-1599 as a bit mask: twc = -Rcw^T tcw, tlc = Rlw twc + tlw, one gemm each."""
    R, t = cam["Rcw"].astype(f64).reshape(3, 3), cam["tcw"].astype(f64)
    twc = np.array([f32(-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2])) for k in range(3)], f32).astype(f64)
    Rl, tl = cam["Rlw"].astype(f64).reshape(3, 3), cam["tlw"].astype(f64)
    z = f32(((Rl[2, 0] * twc[0] + Rl[2, 1] * twc[1]) + Rl[2, 2] * twc[2]) + tl[2])
    mono = bool(cam["mono"])
    return (FORWARD if z > f32(cam["mb"]) and not mono else 0) | (BACKWARD if -z > f32(cam["mb"]) and not mono else 0)


def project(points, cam, n_levels, bounds):
    """-> (query records [hb.PROJ_QUERY, every point], projected u8, status).  u, v, invz hold where projected, zeros elsewhere."""
    points = np.ascontiguousarray(points, LAST_POINT)
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    n = len(points)
    q = np.zeros(n, hb.PROJ_QUERY)
    q["octave"], q["angle"], q["desc"] = points["octave"], points["angle"], points["desc"]
    q["has_obs"] = (points["flags"] & HAS_OBS) != 0
    projected = np.zeros(n, np.uint8)
    status = 0
    R, t = cam["Rcw"].astype(f64).reshape(3, 3), cam["tcw"].astype(f64)
    fx, fy, cx, cy = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        for i in range(n):
            if points["flags"][i] & SKIP:
                continue
            P = points["pos"][i].astype(f64)
            xc, yc, zc = (f32(((R[r, 0] * P[0] + R[r, 1] * P[1]) + R[r, 2] * P[2]) + t[r]) for r in range(3))
            invz = f32(f64(1.0) / f64(zc))
            if invz < 0:
                continue
            u = f32(f32(fx * xc) * invz) + cx
            v = f32(f32(fy * yc) * invz) + cy
            if not (np.isfinite(u) and np.isfinite(v)):
                status |= 1
                continue
            if u < min_x or u > max_x or v < min_y or v > max_y:
                continue
            if points["octave"][i] < 0 or points["octave"][i] >= n_levels:
                status |= 2
                continue
            q["u"][i], q["v"][i], q["invz"][i] = u, v, invz
            projected[i] = 1
    return q, projected, status


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1866-1908) on the bins' sizes -> (ind1, ind2, ind3)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        s = int(s)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def oracle_three_maxima(sizes):
    h = np.ascontiguousarray(sizes, np.int32)
    i1, i2, i3 = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    ob.lib().orc_three_maxima(hb._p(h), C.c_int(len(h)), C.byref(i1), C.byref(i2), C.byref(i3))
    return i1.value, i2.value, i3.value


def rotation_bin(angle_last, angle_cur):
    rot = f32(angle_last) - f32(angle_cur)
    if rot < 0.0:
        rot = rot + f32(360.0)
    x = float(f32(rot * (f32(HISTO_LENGTH) / f32(360.0))))
    b = int(math.copysign(math.floor(abs(x) + 0.5), x))  # roundf: halves away from zero
    return 0 if b == HISTO_LENGTH else b


def search_python(kps, desc, u_right, queries, scale_factors, mbf, th, forward, backward, check_ori, bounds):
    """The greedy loop of ORBmatcher.cc:1595-1702 and the pruning of :1706-1726 in plain Python, from the empty frame; only the window
    (Frame::GetFeaturesInArea) is the oracle's.  -> (nmatches, match [len(kps)] = query index or -1, n_researched: the points whose entry
    best and entry second best -- the best two of their window in the empty frame, a distance of 256 never being one -- are both taken
    when their turn comes, as include/amos_frontend.h states it)."""
    queries = np.ascontiguousarray(queries, hb.PROJ_QUERY)
    view, keep = hb.frame_view(kps, desc, u_right, tuple(float(b) for b in bounds))
    sf = np.asarray(scale_factors, f32)
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.int16)
    match = np.full(len(kps), -1, np.int32)
    taken = np.zeros(len(kps), bool)
    entries = []  # one (feature, bin) per accepted point
    nmatches = both_taken = 0
    for i, p in enumerate(queries):
        octave = int(p["octave"])
        radius = f32(th) * sf[octave]
        lo, hi = (octave, -1) if forward else (0, octave) if backward else (octave - 1, octave + 1)
        cand = hb.oracle_features_in_area(view, float(p["u"]), float(p["v"]), float(radius), lo, hi)
        pbits = np.unpackbits(p["desc"]).astype(np.int16)
        free, everything = [], []
        for i2 in cand:
            if u_right is not None and u_right[i2] > 0:
                ur = f32(p["u"]) - f32(f32(mbf) * f32(p["invz"]))
                if abs(f32(ur - f32(u_right[i2]))) > radius:
                    continue
            d = int(np.abs(bits[i2] - pbits).sum())
            if d >= 256:  # strict < from 256: never a best or a second best
                continue
            everything.append((d, i2))
            if not taken[i2]:
                free.append((d, i2))
        if len(everything) >= 2:
            order = sorted(range(len(everything)), key=lambda k: (everything[k][0], k))
            both_taken += bool(taken[everything[order[0]][1]] and taken[everything[order[1]][1]])
        best_dist, best = 256, -1
        for d, i2 in free:
            if d < best_dist:
                best_dist, best = d, i2
        if best_dist <= TH_HIGH:
            match[best] = i
            nmatches += 1
            if p["has_obs"]:
                taken[best] = True
            if check_ori:
                entries.append((best, rotation_bin(p["angle"], kps["angle"][best])))
    if check_ori:
        winners = three_maxima(np.bincount([b for _, b in entries], minlength=HISTO_LENGTH))
        for i2, b in entries:
            if b not in winners:
                match[i2] = -1
                nmatches -= 1
    return nmatches, match, both_taken


def search_oracle(kps, desc, u_right, queries, scale_factors, mbf, th, forward, backward, check_ori, bounds):
    view, keep = hb.frame_view(kps, desc, u_right, tuple(float(b) for b in bounds))
    n, m = hb.search_frame("oracle", view, queries, np.full(len(kps), -1, np.int32), scale_factors, float(mbf), float(th), int(bool(forward)),
                           int(bool(backward)), check_ori=bool(check_ori))
    return n, m, None


def search_projected(kps, desc, u_right, queries, scale_factors, mbf, th, th_retry, retry_below, forward, backward, check_ori, bounds,
                     impl=search_oracle):
    """Tracking.cc:1925-1945 on projected records: the search from the empty frame, and again with th_retry when it returned fewer than
    retry_below.  -> dict(match [len(kps)] = index into `queries` or -1, n_matches, n_first, pass)."""
    if len(queries) == 0 or len(kps) == 0:
        return {"match": np.full(len(kps), -1, np.int32), "n_matches": 0, "n_first": 0, "pass": 2 if retry_below > 0 else 1}
    n, m, _ = impl(kps, desc, u_right, queries, scale_factors, mbf, th, forward, backward, check_ori, bounds)
    out = {"match": m, "n_matches": int(n), "n_first": int(n), "pass": 1}
    if n < retry_below:
        n, m, _ = impl(kps, desc, u_right, queries, scale_factors, mbf, th_retry, forward, backward, check_ori, bounds)
        out.update(match=m, n_matches=int(n))
        out["pass"] = 2
    return out


def search_motion_model(kps, desc, u_right, points, cam, scale_factors, bounds, impl=search_oracle):
    """-> dict(query, projected, match [len(kps)] = index into `points` or -1, n_projected, n_matches, n_first, pass, flags, status)."""
    q, projected, status = project(points, cam, len(scale_factors), bounds)
    flags = motion_flags(cam)
    idx = np.nonzero(projected)[0]
    r = search_projected(kps, desc, u_right, q[idx], scale_factors, float(cam["mbf"]), float(cam["th"]), float(cam["th_retry"]),
                         int(cam["retry_below"]), flags & FORWARD, flags & BACKWARD, int(cam["check_orientation"]), bounds, impl)
    m = r["match"]
    match = np.where(m >= 0, idx[np.maximum(m, 0)] if len(idx) else -1, -1).astype(np.int32)
    return dict(query=q, projected=projected, match=match, n_projected=int(projected.sum()), n_matches=r["n_matches"], n_first=r["n_first"],
                flags=flags, status=status, **{"pass": r["pass"]})


def researched(kps, desc, u_right, cam, scale_factors, bounds, result):
    """n_researched of a search_motion_model result: search_python's count for the pass that stands, once it has reproduced that pass."""
    idx = np.nonzero(result["projected"])[0]
    if len(idx) == 0 or len(kps) == 0:
        return 0
    flags = result["flags"]
    n, m, both_taken = search_python(kps, desc, u_right, result["query"][idx], scale_factors, float(cam["mbf"]),
                                     float(cam["th_retry"] if result["pass"] == 2 else cam["th"]), flags & FORWARD, flags & BACKWARD,
                                     int(cam["check_orientation"]), bounds)
    assert n == result["n_matches"] and np.array_equal(np.where(m >= 0, idx[np.maximum(m, 0)], -1), result["match"])
    return both_taken


# ---------------------------------------------------------------------------------------------------------------- scenes

def pose(rx, ry, rz, t):
    cx_, sx, cy_, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(f32), np.asarray(t, f32)


def moved(last, rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    """The current pose Tcw = Tcl * Tlw for a motion Tcl given by its angles and translation (the camera moves by -Rcl^T t in the last
    frame's axes: t = (0, 0, -d) is d forward)."""
    Rlw, tlw = last
    Rcl, tcl = pose(rx, ry, rz, t)
    return (Rcl.astype(f64) @ Rlw.astype(f64)).astype(f32), (Rcl.astype(f64) @ tlw.astype(f64) + tcl.astype(f64)).astype(f32)


MOTIONS = {"sideways": dict(t=(0.015, -0.01, 0.005), ry=0.002), "forward": dict(t=(0.0, 0.0, -0.03), rx=0.001),
           "backward": dict(t=(0.002, 0.0, 0.03)), "mono": dict(t=(0.0, 0.0, -0.03))}
MOTION_FLAGS = {"sideways": 0, "forward": FORWARD, "backward": BACKWARD, "mono": 0}


def make_last_points(rng, last_kps, last_desc, m, last_pose, intr, skip_share=0.1, replace=True):
    """m last-frame features with their map points: keypoints of the last frame, drawn with replacement (several points then contest one
    feature of the current frame; replace=False: point i belongs to keypoint i), back-projected at seeded depths through the last pose.  About 70 % of the points have observations,
    `skip_share` carry the skip flag, a few bits of the descriptors are flipped, and point 0 (when there is more than one) lies behind the
    camera."""
    pts = np.zeros(m, LAST_POINT)
    if m == 0:
        return pts
    fx, fy, cx, cy = intr
    pick = rng.integers(0, len(last_kps), m) if replace else np.arange(m)
    k = last_kps[pick]
    z = rng.uniform(2.0, 6.0, m)
    if m > 1:
        z[0] = -z[0]
    x = (k["x"].astype(f64) + rng.normal(0, 0.5, m) - cx) / fx * z
    y = (k["y"].astype(f64) + rng.normal(0, 0.5, m) - cy) / fy * z
    R, t = last_pose[0].astype(f64), last_pose[1].astype(f64)
    pts["pos"] = ((np.stack([x, y, z], 1) - t) @ R).astype(f32)  # R^T (Pl - t)
    pts["angle"], pts["octave"] = k["angle"], k["octave"]
    pts["flags"] = np.where(rng.random(m) < 0.7, HAS_OBS, 0) | np.where(rng.random(m) < skip_share, SKIP, 0)
    pts["desc"] = last_desc[pick]
    flip = rng.random((m, 32)) < 0.02
    pts["desc"] ^= (flip * (1 << rng.integers(0, 8, (m, 32)))).astype(np.uint8)
    return pts


# ---------------------------------------------------------------------------------------------------------------- hand cases

HAND_BOUNDS = (0.0, 640.0, 0.0, 480.0)
HAND_SCALE = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)]).astype(f32)).astype(f32)  # mvScaleFactor as ORBextractor.cc:505-510 builds it


def hand_frame(angles=None):
    """54 level-0 features on a lattice 60 px apart (a window of radius 14 holds one of them) with seeded descriptors: two of them are
    ~128 bits apart, far beyond TH_HIGH."""
    kps = np.zeros(54, hb.KP)
    ii, jj = np.meshgrid(np.arange(9), np.arange(6), indexing="ij")
    kps["x"], kps["y"] = 60.0 + 60.0 * ii.reshape(-1), 60.0 + 60.0 * jj.reshape(-1)
    kps["size"], kps["octave"] = 31.0, 0
    if angles is not None:
        kps["angle"] = angles
    desc = np.random.default_rng(54).integers(0, 256, (54, 32), dtype=np.uint8)
    return kps, desc


def hand_query(kps, desc, feature, angle=0.0, has_obs=0, du=0.0, flip_bits=0):
    """One projected record aimed at `feature`: its position (+ du in x), level 0, its descriptor with the first `flip_bits` bits flipped."""
    q = np.zeros(1, hb.PROJ_QUERY)
    q["u"], q["v"], q["invz"] = kps["x"][feature] + du, kps["y"][feature], 1.0
    q["octave"], q["angle"], q["has_obs"] = 0, angle, has_obs
    d = desc[feature].copy()
    for b in range(flip_bits):
        d[b // 8] ^= 1 << (b % 8)
    q["desc"] = d
    return q
