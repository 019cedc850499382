"""Synthetic frames for the PoseOptimization tests (CPU and GPU): TUM fr3 intrinsics, map points at 0.5 - 8 m, 0 - 1 px of observation
noise, a start pose off by up to 3 degrees / 5 cm; plus the hand-made frames that reach the odd branches."""
import math

import numpy as np

import pose_optimization_restatement as pr

FX, FY, CX, CY, BF = 535.4, 539.2, 320.1, 247.6, 40.0
N_LEVELS = 8
INV_SIGMA2 = np.array([1.0 / (1.2 ** l) ** 2 for l in range(N_LEVELS)], np.float32)
EDGE_COUNTS = (2, 3, 9, 10, 63, 64, 65, 255, 256, 257, 300, 1000)
KINDS = ("mono", "stereo", "mixed")


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def camera(R, t, fx=FX, fy=FY, cx=CX, cy=CY, bf=BF):
    c = np.zeros(1, pr.CAMERA)[0]
    c["Rcw"], c["tcw"] = np.asarray(R, np.float32).reshape(9), np.asarray(t, np.float32)
    c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"] = fx, fy, cx, cy, bf
    return c


def make_case(n_edges, kind="mixed", outliers=0.0, seed=0, extra=None):
    """-> dict(kps, u_right, match, pos [points][3], has_obs [points], camera (the start pose), inv_sigma2, count, R_true, t_true, noise)"""
    rng = np.random.default_rng(seed * 7919 + n_edges * 13 + KINDS.index(kind))
    n = n_edges + n_edges // 3 + 4                      # features; the unmatched ones are spread among the matched
    n_points = n_edges + 5
    R_true = rot(*rng.uniform(-0.2, 0.2, 3))
    t_true = rng.uniform(-0.5, 0.5, 3)
    noise = rng.uniform(0.0, 1.0)
    u, v = rng.uniform(20, 620, n_points), rng.uniform(20, 460, n_points)
    z = rng.uniform(0.5, 8.0, n_points)
    Xc = np.stack([(u - CX) * z / FX, (v - CY) * z / FY, z], 1)
    pos = ((Xc - t_true) @ R_true).astype(np.float32)   # R^T (Xc - t), row-wise
    feats = np.sort(rng.choice(n, n_edges, replace=False))
    pts = rng.permutation(n_points)[:n_edges]
    kps = np.zeros(n, pr.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    kps["octave"] = rng.integers(0, N_LEVELS, n)
    ur = np.full(n, -1.0, np.float32)
    match = np.full(n, -1, np.int32)
    match[feats] = pts
    kps["x"][feats] = u[pts] + rng.normal(0, noise, n_edges)
    kps["y"][feats] = v[pts] + rng.normal(0, noise, n_edges)
    stereo = {"mono": np.zeros(n_edges, bool), "stereo": np.ones(n_edges, bool), "mixed": rng.random(n_edges) < 0.5}[kind]
    ur[feats[stereo]] = (u[pts] - BF / z[pts] + rng.normal(0, noise, n_edges))[stereo]
    gross = feats[rng.random(n_edges) < outliers]
    kps["x"][gross], kps["y"][gross] = rng.uniform(0, 640, len(gross)), rng.uniform(0, 480, len(gross))
    ur[gross] = np.where(ur[gross] < 0, -1.0, kps["x"][gross] - rng.uniform(0, 40, len(gross)))
    dR = rot(*(rng.uniform(-1, 1, 3) * math.radians(3.0) / math.sqrt(3.0)))
    dt = rng.uniform(-1, 1, 3) * 0.05 / math.sqrt(3.0)
    has_obs = rng.random(n_points) < 0.8
    case = dict(kps=kps, u_right=ur, match=match, pos=pos, has_obs=has_obs, camera=camera(dR @ R_true, dR @ t_true + dt), inv_sigma2=INV_SIGMA2,
                count=n, R_true=R_true, t_true=t_true, noise=noise, gross=gross)
    if extra:
        extra(case, rng)
    return case


def grid_cases():
    """the edge counts x kinds x (0 %, 25 % outliers) of the issue -> {name: case}"""
    out = {}
    for n in EDGE_COUNTS:
        for kind in KINDS:
            for frac in (0.0, 0.25):
                out[f"{n}_{kind}_{int(frac * 100)}"] = make_case(n, kind, frac, seed=1)
    return out


def exact_optimum():
    """Every residual is exactly 0.0 at the start pose (identity, power-of-two geometry): b = 0, x = 0, tempChi == currentChi, rho == 0."""
    ks = [(-20 + 3 * i, -15 + 2 * i) for i in range(14)]
    n = len(ks)
    kps = np.zeros(n, pr.KP_DTYPE)
    pos = np.zeros((n, 3), np.float32)
    ur = np.full(n, -1.0, np.float32)
    for i, (a, b) in enumerate(ks):
        z = float(2 ** (i % 3))
        pos[i] = [a / 64.0 * z, b / 64.0 * z, z]
        kps["x"][i], kps["y"][i] = 512.0 * a / 64.0 + 320.0, 512.0 * b / 64.0 + 240.0
        if i % 2:
            ur[i] = kps["x"][i] - 32.0 / z
    kps["octave"] = np.arange(n) % 2 * 0
    return dict(kps=kps, u_right=ur, match=np.arange(n, dtype=np.int32), pos=pos, has_obs=np.ones(n, bool),
                camera=camera(np.eye(3), np.zeros(3), 512.0, 512.0, 320.0, 240.0, 32.0), inv_sigma2=INV_SIGMA2, count=n)


def _on_a_line(case, rng):
    """all points on one line through the camera centre of the START pose"""
    R, t = case["camera"]["Rcw"].astype(np.float64).reshape(3, 3), case["camera"]["tcw"].astype(np.float64)
    d = np.array([0.1, -0.05, 1.0])
    z = rng.uniform(0.5, 8.0, len(case["pos"]))
    case["pos"][:] = ((d[None, :] * z[:, None] - t) @ R).astype(np.float32)
    m = case["match"] >= 0
    case["kps"]["x"][m] = CX + FX * 0.1 + rng.normal(0, 0.5, m.sum())
    case["kps"]["y"][m] = CY - FY * 0.05 + rng.normal(0, 0.5, m.sum())
    case["u_right"][:] = -1.0


def _zero_depth(case, rng):
    """identity start pose and one matched point with Z == 0: z_c == 0 exactly"""
    case["camera"] = camera(np.eye(3), np.zeros(3))
    case["pos"][case["match"][case["match"] >= 0][3], 2] = 0.0


def _behind(case, rng):
    """every fifth matched point mirrored behind the camera"""
    idx = case["match"][case["match"] >= 0][::5]
    R, t = case["R_true"], case["t_true"]
    Xc = case["pos"][idx].astype(np.float64) @ R.T + t
    case["pos"][idx] = ((-Xc - t) @ R).astype(np.float32)


def _bad_octave(case, rng):
    f = np.nonzero(case["match"] >= 0)[0]
    case["kps"]["octave"][f[2]] = N_LEVELS + 1
    case["kps"]["octave"][f[5]] = -1


def _bad_match_index(case, rng):
    f = np.nonzero(case["match"] >= 0)[0]
    case["match"][f[4]] = len(case["pos"]) + 3


def _no_features(case, rng):
    case["count"] = 0


def special_cases():
    return {
        "exact_optimum": exact_optimum(),
        "line_mono": make_case(40, "mono", 0.0, seed=2, extra=_on_a_line),
        "zero_depth_mono": make_case(64, "mono", 0.0, seed=3, extra=_zero_depth),
        "zero_depth_stereo": make_case(64, "stereo", 0.0, seed=3, extra=_zero_depth),
        "behind": make_case(120, "mixed", 0.0, seed=4, extra=_behind),
        "bad_octave": make_case(50, "mixed", 0.25, seed=5, extra=_bad_octave),
        "bad_match_index": make_case(50, "mixed", 0.0, seed=6, extra=_bad_match_index),
        "count_zero": make_case(30, "mixed", 0.0, seed=7, extra=_no_features),
    }


def negative_sigma_case():
    """a table of NEGATIVE weights (no frame has one): H is negative definite, every pivot is negative, every solve fails"""
    c = make_case(40, "mixed", 0.0, seed=8)
    c["inv_sigma2"] = -INV_SIGMA2
    return c


def all_cases():
    out = grid_cases()
    out.update(special_cases())
    return out


def restate(case, clear_outliers=0, fill=7):
    """the restatement on one case -> (RESULT record, outlier bytes [features], match [features])"""
    return pr.pose_optimization(case["kps"], case["u_right"], case["match"], case["pos"], case["has_obs"], case["camera"], case["inv_sigma2"],
                                np.full(len(case["kps"]), fill, np.uint8), clear_outliers, case["count"])


def pose_optimization_with_entry(case, entry):
    """the restatement with mvbOutlier = entry on entry and no discard loop (what the drop-in sees)"""
    return pr.pose_optimization(case["kps"], case["u_right"], case["match"], case["pos"], case["has_obs"], case["camera"], case["inv_sigma2"],
                                np.array(entry, np.uint8), 0, case["count"])


def same_bits(a, b):
    """equal bit for bit, or NaN on both sides (a NaN's sign and payload differ between processors and are not part of the arithmetic)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and bool((a == b).all())
    ai, bi = a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}")
    return a.shape == b.shape and bool(((ai == bi) | (np.isnan(a) & np.isnan(b))).all())
