"""Step 2 of Tracking::SearchLocalPoints restated in numpy for the tests: Frame::isInFrustum + MapPoint::PredictScale exactly as
include/amos_frontend.h ("local map search") defines their arithmetic -- float32 operation by operation, float64 where the definition says
so -- then ORBmatcher::SearchByProjection(F, vpMapPoints, th) by the CPU oracle (orc_search_by_projection_points) on the records in view.
Also the seeded scenes the CPU and GPU tests share."""
import numpy as np

import host_binding as hb

MAP_POINT = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"),
                      ("flags", "<i4"), ("desc", "u1", (32,)), ("pad", "u1", (12,))])
CAMERA = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                   ("cy", "<f4"), ("mbf", "<f4"), ("view_cos_limit", "<f4"), ("th", "<f4"), ("nn_ratio", "<f4")])
SKIP, HAS_OBS = 1, 2
f32, f64 = np.float32, np.float64
REASONS = {"skip": 1, "behind": 2, "not_finite": 3, "outside": 4, "near": 5, "far": 6, "angle": 7}


def table_level(ratio, scale_factors):
    """PredictScale without a logarithm: how many table entries the ratio exceeds, at most n_levels - 1 (NaN: 0)."""
    ratio = np.asarray(ratio, f32)
    sf = np.asarray(scale_factors, f32)
    with np.errstate(invalid="ignore"):
        level = (ratio[..., None] > sf).sum(-1)
    return np.minimum(level, len(sf) - 1).astype(np.int32)


def frustum(points, cam, scale_factors, bounds):
    """-> (query records [MAP_QUERY, every point], in_view u8, status, reason).  Records hold the projection where in view, zeros elsewhere;
    reason names the branch that rejected a point (REASONS), 0 where in view."""
    points = np.ascontiguousarray(points, MAP_POINT)
    sf = np.asarray(scale_factors, f32)
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    n = len(points)
    q = np.zeros(n, hb.MAP_QUERY)
    q["has_obs"] = (points["flags"] & HAS_OBS) != 0
    q["desc"] = points["desc"]
    in_view = np.zeros(n, np.uint8)
    reason = np.zeros(n, np.int8)
    status = 0
    R, t, Ow = cam["Rcw"].astype(f64).reshape(3, 3), cam["tcw"].astype(f64), cam["Ow"].astype(f32)
    with np.errstate(all="ignore"):
        for i in range(n):
            if points["flags"][i] & SKIP:
                reason[i] = REASONS["skip"]
                continue
            P = points["pos"][i].astype(f32)
            Pd = P.astype(f64)
            Pc = [f32(((R[r, 0] * Pd[0] + R[r, 1] * Pd[1]) + R[r, 2] * Pd[2]) + t[r]) for r in range(3)]
            if Pc[2] < f32(0):
                reason[i] = REASONS["behind"]
                continue
            invz = f32(1) / Pc[2]
            u = f32(f32(f32(cam["fx"]) * Pc[0]) * invz) + f32(cam["cx"])
            v = f32(f32(f32(cam["fy"]) * Pc[1]) * invz) + f32(cam["cy"])
            if not (np.isfinite(u) and np.isfinite(v)):
                status = 1
                reason[i] = REASONS["not_finite"]
                continue
            if u < min_x or u > max_x or v < min_y or v > max_y:
                reason[i] = REASONS["outside"]
                continue
            PO = (P - Ow).astype(f32)
            POd = PO.astype(f64)
            dist = f32(np.sqrt((POd[0] * POd[0] + POd[1] * POd[1]) + POd[2] * POd[2]))
            if dist < f32(0.8) * points["min_distance"][i] or dist > f32(1.2) * points["max_distance"][i]:
                reason[i] = REASONS["near"] if dist < f32(0.8) * points["min_distance"][i] else REASONS["far"]
                continue
            Pn = points["normal"][i].astype(f64)
            view_cos = f32(((POd[0] * Pn[0] + POd[1] * Pn[1]) + POd[2] * Pn[2]) / f64(dist))
            if view_cos < f32(cam["view_cos_limit"]):
                reason[i] = REASONS["angle"]
                continue
            ratio = f32(points["max_distance"][i]) / dist
            q["proj_x"][i], q["proj_y"][i] = u, v
            q["proj_xr"][i] = u - f32(f32(cam["mbf"]) * invz)
            q["view_cos"][i] = view_cos
            q["level"][i] = table_level(ratio, sf)
            in_view[i] = 1
    return q, in_view, status, reason


def search_python(view, kps, desc, u_right, queries, occupied, scale_factors, th, nn_ratio):
    """The greedy loop of ORBmatcher.cc:77-172 in plain Python; only the window (Frame::GetFeaturesInArea) is the oracle's.  Beside the
    live loop it keeps each point's ENTRY record: the best two of its window against the frame as it stands on entry (`occupied`).
    -> (nmatches, match [len(kps)] = query index or -1, n_researched: the points that have a candidate on entry and whose entry best or
    entry second best is taken when their turn comes, as include/amos_frontend.h states it)."""
    sf = np.asarray(scale_factors, f32)
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1)
    taken = np.asarray(occupied, np.uint8) != 0
    entry_free = ~taken
    match = np.full(len(kps), -1, np.int32)
    nmatches = n_researched = 0

    def best_two(cand, dist, free):  # strict <, from 256: the first of equal distances wins, a distance of 256 never does
        order = [k for k in np.argsort(dist, kind="stable") if free[cand[k]] and dist[k] < 256][:2]
        return [(int(cand[k]), int(dist[k])) for k in order]
    for i, p in enumerate(queries):
        level = int(p["level"])
        r = f32(2.5) if float(p["view_cos"]) > 0.998 else f32(4.0)
        if f32(th) != f32(1.0):
            r = f32(r * f32(th))
        r = f32(r * sf[level])
        cand = hb.oracle_features_in_area(view, float(p["proj_x"]), float(p["proj_y"]), float(r), level - 1, level)
        if u_right is not None:
            ur = np.asarray(u_right, f32)[cand]
            cand = cand[~((ur > 0) & (np.abs(f32(p["proj_xr"]) - ur) > r))]
        dist = (bits[cand] != np.unpackbits(p["desc"])).sum(1)
        entry, now = best_two(cand, dist, entry_free), best_two(cand, dist, ~taken)
        n_researched += bool(entry) and any(taken[c] for c, _ in entry)
        if not now or now[0][1] > 100:
            continue
        (best, bd), (second, sd) = now[0], now[1] if len(now) > 1 else (-1, 256)
        if second >= 0 and kps["octave"][best] == kps["octave"][second] and f32(bd) > f32(nn_ratio) * f32(sd):
            continue
        match[best] = i
        taken[best] = p["has_obs"] != 0
        nmatches += 1
    return nmatches, match, int(n_researched)


def search_local_points(kps, desc, u_right, points, cam, occupied, scale_factors, bounds):
    """-> dict(query, in_view, match [len(kps)] = index into `points` or -1, n_in_view, n_matches, n_researched, status): the oracle's
    search, and n_researched from the Python loop once that loop has reproduced the oracle's matches."""
    q, in_view, status, reason = frustum(points, cam, scale_factors, bounds)
    idx = np.nonzero(in_view)[0]
    match = np.full(len(kps), -1, np.int32)
    n_matches = n_researched = 0
    if len(idx) and len(kps):
        view, keep = hb.frame_view(kps, desc, u_right, tuple(float(b) for b in bounds))
        n_matches, m, _ = hb.search_points("oracle", view, q[idx], match, np.asarray(occupied, np.uint8), scale_factors, float(cam["th"]),
                                           float(cam["nn_ratio"]))
        n_py, m_py, n_researched = search_python(view, kps, desc, u_right, q[idx], occupied, scale_factors, cam["th"], cam["nn_ratio"])
        assert n_py == n_matches and np.array_equal(m_py, m)
        match = np.where(m >= 0, idx[np.maximum(m, 0)], -1).astype(np.int32)
    return dict(query=q, in_view=in_view, reason=reason, match=match, n_in_view=int(in_view.sum()), n_matches=int(n_matches),
                n_researched=n_researched, status=status)


# ---------------------------------------------------------------------------------------------------------------- scenes

def pose(rx, ry, rz, t):
    cx_, sx, cy_, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(f32), np.asarray(t, f32)


def camera(R, t, fx, fy, cx, cy, mbf=40.0, view_cos_limit=0.5, th=1.0, nn_ratio=0.8):
    c = np.zeros((), CAMERA)
    c["Rcw"], c["tcw"] = R.reshape(9), t
    c["Ow"] = (-(R.astype(f64).T @ t.astype(f64))).astype(f32)  # Frame::UpdatePoseMatrices: mOw = -Rcw.t() * tcw
    c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"] = fx, fy, cx, cy, mbf
    c["view_cos_limit"], c["th"], c["nn_ratio"] = view_cos_limit, th, nn_ratio
    return c


def make_points(rng, src_kps, src_desc, m, cam, scale_factors, gate_share=0.15):
    """m map points: keypoints of another frame back-projected at seeded depths through the camera's pose, normals toward the camera plus
    noise; max_distance puts the predicted level at the keypoint's octave (or one above), and about `gate_share` of the points fail each
    of the four gates (behind / outside the image, distance range, viewing angle, skip flag)."""
    pts = np.zeros(m, MAP_POINT)
    if m == 0:
        return pts
    sf = np.asarray(scale_factors, f64)
    pick = rng.integers(0, len(src_kps), m)
    k = src_kps[pick]
    z = rng.uniform(1.0, 4.0, m)
    x = (k["x"].astype(f64) + rng.normal(0, 0.7, m) - float(cam["cx"])) / float(cam["fx"]) * z
    y = (k["y"].astype(f64) + rng.normal(0, 0.7, m) - float(cam["cy"])) / float(cam["fy"]) * z
    R, t = cam["Rcw"].astype(f64).reshape(3, 3), cam["tcw"].astype(f64)
    gate = rng.random(m)
    behind = gate < gate_share / 2
    outside = (gate >= gate_share / 2) & (gate < gate_share)
    z = np.where(behind, -z, z)
    x = np.where(outside, x + 3.0 * z, x)
    world = (np.stack([x, y, z], 1) - t) @ R  # R^T (Pc - t)
    pts["pos"] = world.astype(f32)
    Ow = cam["Ow"].astype(f64)
    PO = pts["pos"].astype(f64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    normal = PO / dist[:, None] + rng.normal(0, 0.15, (m, 3))
    away = (gate >= 2 * gate_share) & (gate < 3 * gate_share)  # viewing angle beyond 60 degrees
    side = np.cross(PO / dist[:, None], rng.normal(0, 1, (m, 3)))
    side /= np.linalg.norm(side, axis=1)[:, None]
    normal = np.where(away[:, None], 0.2 * PO / dist[:, None] + side, normal)
    pts["normal"] = (normal / np.linalg.norm(normal, axis=1)[:, None]).astype(f32)
    level = np.minimum(k["octave"] + rng.integers(0, 2, m), len(sf) - 1)
    pts["max_distance"] = (dist * sf[level] * rng.uniform(0.93, 0.99, m)).astype(f32)
    pts["min_distance"] = (pts["max_distance"] / sf[-1] / 1.5).astype(f32)
    far = (gate >= gate_share) & (gate < 1.5 * gate_share)
    near = (gate >= 1.5 * gate_share) & (gate < 2 * gate_share)
    pts["max_distance"] = np.where(far, dist / 1.3, pts["max_distance"]).astype(f32)
    pts["min_distance"] = np.where(near, dist * 1.4, np.where(far, dist / 10, pts["min_distance"])).astype(f32)
    pts["max_distance"] = np.where(near, dist * 3, pts["max_distance"]).astype(f32)
    pts["flags"] = np.where(rng.random(m) < 0.7, HAS_OBS, 0) | np.where((gate >= 3 * gate_share) & (gate < 3.5 * gate_share), SKIP, 0)
    pts["desc"] = src_desc[pick]
    flip = rng.random((m, 32)) < 0.02  # a few bits of descriptor noise
    pts["desc"] ^= (flip * (1 << rng.integers(0, 8, (m, 32)))).astype(np.uint8)
    return pts


def grid_cells(kps, bounds):
    """Frame::PosInGrid (Frame.cc:1007-1030) per keypoint: col * 48 + row, or -1."""
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    winv, hinv = f32(64) / f32(max_x - min_x), f32(48) / f32(max_y - min_y)
    # roundf: half away from zero
    fx, fy = (kps["x"].astype(f32) - min_x) * winv, (kps["y"].astype(f32) - min_y) * hinv
    px = (np.sign(fx) * np.floor(np.abs(fx.astype(f64)) + 0.5)).astype(np.int64)
    py = (np.sign(fy) * np.floor(np.abs(fy.astype(f64)) + 0.5)).astype(np.int64)
    ok = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    return np.where(ok, px * 48 + py, -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- hand cases

HAND_BOUNDS = (0.0, 640.0, 0.0, 480.0)
HAND_SCALE = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)]).astype(f32)).astype(f32)  # mvScaleFactor as ORBextractor.cc:505-510 builds it


def hand_frame():
    """Two level-0 features, 3 px either side of the image centre: inside a window of radius 4, outside one of radius 2.5."""
    kps = np.zeros(2, hb.KP)
    kps["x"], kps["y"], kps["size"], kps["octave"] = [323.0, 317.0], [240.0, 240.0], 31.0, 0
    desc = np.zeros((2, 32), np.uint8)
    desc[1] = 0xFF
    return kps, desc


def hand_cases():
    """name -> (points, camera, expected in_view per point, expected status, expected levels or None, expected matches or None)."""
    R, t = np.eye(3, dtype=f32), np.zeros(3, f32)
    cam = camera(R, t, 512.0, 512.0, 320.0, 240.0)

    def point(pos, normal=None, min_d=0.0, max_d=100.0, flags=HAS_OBS):
        p = np.zeros(1, MAP_POINT)
        p["pos"] = pos
        n = np.asarray(pos, f64) if normal is None else np.asarray(normal, f64)
        p["normal"] = n / max(np.linalg.norm(n), 1e-30) if normal is None else n
        p["min_distance"], p["max_distance"], p["flags"] = min_d, max_d, flags
        return p

    cases = {}
    cases["behind"] = (point([0, 0, -1.0]), cam, [0], 0, None, None)
    cases["nan_projection"] = (point([0, 0, 0.0], normal=[0, 0, 1]), cam, [0], 1, None, None)
    cases["on_min_x_and_max_x"] = (np.concatenate([point([-0.625, 0, 1.0]), point([0.625, 0, 1.0]), point([-0.6251, 0, 1.0]),
                                                   point([0.6251, 0, 1.0])]), cam, [1, 1, 0, 0], 0, None, None)
    # dist = 2 exactly; limits that round to 2 exactly are kept, the next floats beyond are not
    lo = f32(2.5)
    assert f32(0.8) * lo == f32(2.0)
    hi = f32(2.0 / 1.2)
    while f32(1.2) * hi < f32(2.0):
        hi = np.nextafter(hi, f32(9))
    while f32(1.2) * np.nextafter(hi, f32(0)) >= f32(2.0):
        hi = np.nextafter(hi, f32(0))
    assert f32(1.2) * hi == f32(2.0)
    lo_out = lo
    while f32(0.8) * lo_out <= f32(2.0):
        lo_out = np.nextafter(lo_out, f32(9))
    cases["distance_limits"] = (np.concatenate([point([0, 0, 2.0], min_d=lo), point([0, 0, 2.0], min_d=lo_out), point([0, 0, 2.0], max_d=hi),
                                                point([0, 0, 2.0], max_d=np.nextafter(hi, f32(0)))]), cam, [1, 0, 1, 0], 0, None, None)
    half_lo = np.nextafter(f32(0.5), f32(0))

    def tilted(c):  # viewCos = c exactly: PO = (0, 0, 2), dist = 2
        return [float(np.sqrt(1.0 - float(c) ** 2)), 0.0, float(c)]

    cases["view_cos_limit"] = (np.concatenate([point([0, 0, 2.0], normal=tilted(f32(0.5))), point([0, 0, 2.0], normal=tilted(half_lo))]), cam,
                               [1, 0], 0, None, None)
    # 0.998 as a double lies between two floats: the upper one takes the narrow window (no feature within 2.5 px), the lower the wide one
    up = f32(0.998)
    assert float(up) > 0.998 > float(np.nextafter(up, f32(0)))
    cases["radius_narrow"] = (point([0, 0, 2.0], normal=tilted(up), max_d=1.9), cam, [1], 0, [0], [-1, -1])
    cases["radius_wide"] = (point([0, 0, 2.0], normal=tilted(np.nextafter(up, f32(0))), max_d=1.9), cam, [1], 0, [0], [0, -1])
    on = f32(2.0) * HAND_SCALE[3]  # ratio == the table entry: not above it
    cases["levels"] = (np.concatenate([point([0, 0, 2.0], max_d=1.9), point([0, 0, 2.0], max_d=1e6), point([0, 0, 2.0], max_d=on),
                                       point([0, 0, 2.0], max_d=np.nextafter(on, f32(1e9)))]), cam, [1, 1, 1, 1], 0, [0, 7, 3, 4], None)
    return cases
