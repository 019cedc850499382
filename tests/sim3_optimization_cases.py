"""Scenes for the OptimizeSim3 tests: two keyframes with the TUM fr3 intrinsics, map points 0.5 to 8 m in front of both, a true Sim3 of a few
degrees and centimetres with scale 1 (fix_scale = 1) or 0.8 to 1.25 (fix_scale = 0), a start Sim3 off by up to 3 degrees, 5 cm and 3 %,
0 to 1 px of observation noise, unmatched features interleaved, and gross outliers whose reprojection error is far above th2."""
import numpy as np

import sim3_optimization_restatement as so

f32 = np.float32
FX, FY, CX, CY = 535.4, 539.2, 320.1, 247.6
N_LEVELS = 8
INV_SIGMA2 = np.array([1.0 / (1.2 ** l) ** 2 for l in range(N_LEVELS)], f32)
TH2 = 10.0
GRID_COUNTS = (9, 10, 11, 19, 20, 63, 64, 65, 255, 256, 257, 300)


def rot(axis, deg):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def camera(R, t, fx=FX, fy=FY, cx=CX, cy=CY):
    c = np.zeros(1, so.CAMERA)
    c["Rcw"], c["tcw"], c["fx"], c["fy"], c["cx"], c["cy"] = np.asarray(R, f32).reshape(9), t, fx, fy, cx, cy
    return c[0]


def scene(n, fix_scale, outliers=0.0, seed=0, noise=None, extra=True):
    """n correspondences (the gross outliers among them) -> dict(kps1, pts1, cam1, kps2, pts2, cam2, row, pair, truth, is_outlier by
    keyframe-1 feature)"""
    rng = np.random.default_rng(seed * 1000 + n * 4 + fix_scale * 2 + (1 if outliers else 0))
    noise = rng.uniform(0.0, 1.0) if noise is None else noise
    R1w, t1w = rot(rng.normal(size=3), rng.uniform(0, 20)), rng.uniform(-0.5, 0.5, 3)
    R2w, t2w = rot(rng.normal(size=3), rng.uniform(0, 20)), rng.uniform(-0.5, 0.5, 3)
    s = 1.0 if fix_scale else rng.uniform(0.8, 1.25)
    R12, t12 = rot(rng.normal(size=3), rng.uniform(1, 4)), rng.uniform(-0.04, 0.04, 3)
    n1, n2 = (n + n // 3 + 2, n + n // 4 + 3) if extra else (n, n)
    # points in keyframe 1's camera frame, seen by both
    X1, X2 = np.zeros((0, 3)), np.zeros((0, 3))
    while len(X1) < max(n1, n2):
        z = rng.uniform(0.5, 8.0, 4 * max(n1, n2))
        u, v = rng.uniform(40, 600, len(z)), rng.uniform(40, 440, len(z))
        a = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], 1)
        b = (a - t12) @ R12 / s  # S12^-1
        ub, vb = FX * b[:, 0] / b[:, 2] + CX, FY * b[:, 1] / b[:, 2] + CY
        ok = (b[:, 2] > 0.3) & (ub > 20) & (ub < 620) & (vb > 20) & (vb < 460)
        X1, X2 = np.concatenate([X1, a[ok]]), np.concatenate([X2, b[ok]])
    feat1, feat2 = rng.permutation(n1)[:n], rng.permutation(n2)[:n]
    feat1.sort()
    kps1, kps2 = np.zeros(n1, so.KP_DTYPE), np.zeros(n2, so.KP_DTYPE)
    pts1, pts2 = np.zeros(n1, so.POINT), np.zeros(n2, so.POINT)
    for kps, pts, X, Rw, tw, m in ((kps1, pts1, X1, R1w, t1w, n1), (kps2, pts2, X2, R2w, t2w, n2)):
        x = X[:m]
        kps["x"] = FX * x[:, 0] / x[:, 2] + CX + rng.uniform(-noise, noise, m)
        kps["y"] = FY * x[:, 1] / x[:, 2] + CY + rng.uniform(-noise, noise, m)
        kps["octave"] = rng.integers(0, 4, m)
        pts["pos"] = (x - tw) @ Rw  # Rw^T (x - tw)
    # the matched features: keyframe 1's feature feat1[c] and keyframe 2's feature feat2[c] see one physical point
    X1m = X1[:n]
    X2m = (X1m - t12) @ R12 / s
    for c in range(n):
        i, j = feat1[c], feat2[c]
        kps1["x"][i] = FX * X1m[c, 0] / X1m[c, 2] + CX + rng.uniform(-noise, noise)
        kps1["y"][i] = FY * X1m[c, 1] / X1m[c, 2] + CY + rng.uniform(-noise, noise)
        kps2["x"][j] = FX * X2m[c, 0] / X2m[c, 2] + CX + rng.uniform(-noise, noise)
        kps2["y"][j] = FY * X2m[c, 1] / X2m[c, 2] + CY + rng.uniform(-noise, noise)
        pts1["pos"][i] = (X1m[c] - t1w) @ R1w
        pts2["pos"][j] = (X2m[c] - t2w) @ R2w
    row = np.full(n1, -1, np.int32)
    row[feat1] = feat2
    is_outlier = np.zeros(n1, bool)
    n_out = int(round(outliers * n))
    for c in rng.permutation(n)[:n_out]:  # a gross outlier: keyframe 2's observation 30 to 80 px away
        ang, d = rng.uniform(0, 2 * np.pi), rng.uniform(30, 80)
        kps2["x"][feat2[c]] += d * np.cos(ang)
        kps2["y"][feat2[c]] += d * np.sin(ang)
        is_outlier[feat1[c]] = True
    # unmatched features of keyframe 1: some without a point, some matched elsewhere
    free = np.setdiff1d(np.arange(n1), feat1)
    for k, i in enumerate(free):
        if k % 3 == 0:
            pts1["flags"][i] = so.POINT_SKIP
        elif k % 3 == 1:
            row[i] = so.MATCHED_ELSEWHERE
    # the start: the truth off by up to 3 degrees, 5 cm, 3 %
    R0 = rot(rng.normal(size=3), rng.uniform(0.5, 3.0)) @ R12
    t0 = t12 + rng.uniform(-0.03, 0.03, 3)
    s0 = 1.0 if fix_scale else s * rng.uniform(0.97, 1.03)
    return dict(kps1=kps1, pts1=pts1, cam1=camera(R1w, t1w), kps2=kps2, pts2=pts2, cam2=camera(R2w, t2w), row=row,
                pair=so.pair_record(R0, t0, s0, TH2, fix_scale), truth=(R12, t12, s), is_outlier=is_outlier, n=n)


def exact_scene(n=24, fix_scale=0):
    """every residual exactly 0.0 at the start: identity poses and Sim3, power-of-two intrinsics, points whose projections are integers"""
    n1 = n2 = n
    kps1, kps2 = np.zeros(n1, so.KP_DTYPE), np.zeros(n2, so.KP_DTYPE)
    pts1, pts2 = np.zeros(n1, so.POINT), np.zeros(n2, so.POINT)
    for c in range(n):
        z = (1.0, 2.0, 4.0)[c % 3]
        kx, ky = (c * 7) % 33 - 16, (c * 5) % 25 - 12
        X = (z * kx / 64.0, z * ky / 64.0, z)
        pts1["pos"][c] = pts2["pos"][c] = X
        for kps in (kps1, kps2):
            kps["x"][c], kps["y"][c], kps["octave"][c] = 512.0 * kx / 64.0 + 320.0, 512.0 * ky / 64.0 + 240.0, c % 4
    cam = camera(np.eye(3), [0, 0, 0], 512.0, 512.0, 320.0, 240.0)
    return dict(kps1=kps1, pts1=pts1, cam1=cam, kps2=kps2, pts2=pts2, cam2=cam.copy(), row=np.arange(n, dtype=np.int32),
                pair=so.pair_record(np.eye(3), [0, 0, 0], 1.0, TH2, fix_scale), n=n)


def grid():
    """the grid every test shares: every count, both fix_scale values, 0 % and 25 % gross outliers -> [(name, scene)]"""
    return [(f"n{n}_fix{fix}_out{int(out * 100)}", scene(n, fix, out, seed=1)) for n in GRID_COUNTS for fix in (0, 1) for out in (0.0, 0.25)]


def expected(sc, n1=None, n2=None):
    return so.sim3_optimize(sc["kps1"], sc["pts1"], sc["cam1"], sc["kps2"], sc["pts2"], sc["cam2"], sc["row"], INV_SIGMA2, sc["pair"], n1, n2)


_shared = None


def shared():
    """the grid and its restatement results, computed once: ([(name, scene)], [(result, row)])"""
    global _shared
    if _shared is None:
        g = grid()
        _shared = (g, [expected(sc) for _, sc in g])
    return _shared
