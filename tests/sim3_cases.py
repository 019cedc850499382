"""tests/sim3_cases.py -- the synthetic keyframe pairs of the loop-closing Sim3 tests, shared by tests/test_sim3_cpu.py (host-compiled
solver, drop-in constructor), tests/test_gpu_sim3.py (kernel) and tests/test_gpu_sim3_host.py (drop-in): two cameras, points in front of
both, a known (s, R, t) with X1c = s R X2c + t, pixel noise applied by perturbing keyframe 2's points, a stated share of gross outliers,
octaves spread over an 8-level table -- and the restatement's calls on each, computed once per case.  The file itself asserts (at the end,
when it is imported, with the restatement on the CPU) that its seeds do what the cases are named for: if a seed stops doing so, change the seed."""
import functools

import numpy as np

import sim3_restatement as sr

CAPACITY = 64
N_FEATURES = 64
LEVEL_SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], np.float32)
REFERENCE = dict(probability=0.99, min_inliers=20, max_iterations=300)  # LoopClosing.cc:390
N_CALLS, N_ITERATIONS = 3, 5
ROUND = 64  # the kernel's drawn-ahead iterations per round (kS3Round)
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
POINT = np.dtype([("pos", "<f4", (3,)), ("flags", "<i4")])
CAMERA = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])
K1, K2 = (517.3, 516.5, 318.6, 255.3), (520.9, 521.0, 325.1, 249.7)
f32 = np.float32


def rotation(axis, angle):
    """Rodrigues' formula in float64."""
    axis = np.asarray(axis, np.float64)
    k = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def camera(R, t, K):
    c = np.zeros(1, CAMERA)
    c["Rcw"], c["tcw"] = np.asarray(R, np.float64).reshape(9), t
    c["fx"], c["fy"], c["cx"], c["cy"] = K
    return c[0]


TRUTH = (1.15, rotation((0.3, -1.0, 0.2), 0.25), np.array([0.30, -0.10, 0.20]))

# name: dict(nc correspondences, outliers share, noise pixels, kind, scene seed, generator seed, params, n_calls, n_iterations, fix_scale)
CASES = {
    "three_calls": dict(nc=60, outliers=0.4, noise=0.5, scene=1, seed=8),
    "three_calls_fix_scale": dict(nc=60, outliers=0.4, noise=0.5, scene=2, seed=16, fix_scale=1),
    "early_stop_in_round": dict(nc=60, outliers=0.4, noise=0.5, scene=3, seed=1, n_calls=1, n_iterations=300),
    "two_rounds_no_success": dict(nc=60, outliers=0.75, noise=0.0, scene=4, seed=1, n_calls=1, n_iterations=300),
    "noise_free": dict(nc=40, outliers=0.0, noise=0.0, scene=5, seed=9),
    "n_equals_min_inliers": dict(nc=20, outliers=0.0, noise=0.0, scene=6, seed=13),
    "n_below_min_inliers": dict(nc=19, outliers=0.0, noise=0.0, scene=7, seed=17),
    "n24": dict(nc=24, outliers=0.0, noise=0.5, scene=8, seed=19),
    "degenerate": dict(nc=24, outliers=1.0, noise=0.0, scene=9, seed=1, kind="degenerate", n_calls=1, n_iterations=300,
                       params=dict(REFERENCE, min_inliers=6)),
    "pure_translation": dict(nc=24, outliers=0.0, noise=0.0, scene=10, seed=23, kind="translation", n_calls=1, n_iterations=300, fix_scale=1),
}


def make_pair(nc, outliers, noise, scene, kind="", n_features=N_FEATURES, skipped=4, truth=TRUTH, fix_scale=0, cams=None):
    """-> dict(kps1, points1, cam1, kps2, points2, cam2, match12, truth, inlier_truth [nc])."""
    rng = np.random.default_rng(7000 + scene)
    s, R, t = truth
    if fix_scale:
        s = 1.0
    n1 = n2 = n_features
    if kind in ("translation", "degenerate"):  # camera coordinates are world coordinates: exact values survive the constructor
        cam1, cam2 = camera(np.eye(3), np.zeros(3), K1), camera(np.eye(3), np.zeros(3), K2)
    elif cams is not None:
        cam1, cam2 = cams
    else:
        cam1 = camera(rotation((0.1, 0.9, 0.3), 0.4), np.array([0.2, -0.3, 0.5]), K1)
        cam2 = camera(rotation((-0.5, 0.2, 0.7), -0.3), np.array([-0.4, 0.1, 0.3]), K2)
    z = rng.uniform(2.0, 8.0, nc)
    u, v = rng.uniform(120, 520, nc), rng.uniform(100, 380, nc)
    X1 = np.stack([(u - K1[2]) / K1[0] * z, (v - K1[3]) / K1[1] * z, z], 1)
    if kind == "translation":  # every coordinate a multiple of 3 / 64 and R = I, s = 1: centroids and relative coordinates are exact, M is
        R, s = np.eye(3), 1.0  # exactly symmetric and the quaternion's imaginary part exactly 0
        t = np.array([24, -9, 15]) * (3.0 / 64.0)
        X1 = np.round(X1 * (64.0 / 3.0)) * (3.0 / 64.0)
    X2 = (X1 - t) @ R / s  # R^T (X1 - t) / s, row-wise
    inlier_truth = np.ones(nc, bool)
    n_out = int(round(outliers * nc))
    bad = rng.choice(nc, n_out, replace=False)
    inlier_truth[bad] = False
    zo = rng.uniform(2.0, 8.0, n_out)
    X2[bad] = np.stack([rng.uniform(-0.4, 0.4, n_out) * zo, rng.uniform(-0.3, 0.3, n_out) * zo, zo], 1)
    if noise:
        X2[:, :2] += rng.normal(0, noise, (nc, 2)) * (X2[:, 2:3] / float(cam2["fx"]))
    if kind == "degenerate" and nc >= 16:
        X1[1] = X1[2] = X1[0]  # three coincident correspondences
        X2[1] = X2[2] = X2[0]
        for k in range(1, 6):  # six collinear ones
            X1[3 + k] = X1[3] + k * np.array([0.25, 0.125, 0.5])
            X2[3 + k] = X2[3] + k * np.array([0.125, -0.25, 0.375])
        X2[10, 2] = 0.0  # a point with z = 0 in camera 2
        X1[11, 2] = 0.0  # and one in camera 1
    Rc1, tc1 = cam1["Rcw"].reshape(3, 3).astype(np.float64), cam1["tcw"].astype(np.float64)
    Rc2, tc2 = cam2["Rcw"].reshape(3, 3).astype(np.float64), cam2["tcw"].astype(np.float64)
    W1, W2 = (X1 - tc1) @ Rc1, (X2 - tc2) @ Rc2  # Rcw^T (Xc - tcw)
    kps1, kps2 = np.zeros(n1, KP), np.zeros(n2, KP)
    for kps in (kps1, kps2):
        kps["x"], kps["y"] = rng.uniform(0, 640, len(kps)).astype(f32), rng.uniform(0, 480, len(kps)).astype(f32)
        kps["octave"] = rng.integers(0, 8, len(kps))
        kps["size"], kps["angle"] = 31.0, rng.uniform(0, 360, len(kps))
    points1, points2 = np.zeros(n1, POINT), np.zeros(n2, POINT)
    points1["pos"], points2["pos"] = rng.uniform(-3, 3, (n1, 3)), rng.uniform(-3, 3, (n2, 3))
    points1["flags"][rng.choice(n1, n1 // 8, replace=False)] = sr.POINT_SKIP  # features without a point
    points2["flags"][rng.choice(n2, n2 // 8, replace=False)] = sr.POINT_SKIP
    m = min(nc + skipped, n1)
    skipped = m - nc
    feats1 = np.sort(rng.choice(n1, m, replace=False))
    feats2 = rng.choice(n2, m, replace=False)
    is_skip = np.zeros(m, bool)
    is_skip[rng.choice(m, skipped, replace=False)] = True
    match12 = np.full(n1, -1, np.int32)
    match12[feats1] = feats2
    good1, good2 = feats1[~is_skip], feats2[~is_skip]
    points1["pos"][good1], points2["pos"][good2] = W1, W2
    points1["flags"][good1] = points2["flags"][good2] = 0
    for k, i in enumerate(np.nonzero(is_skip)[0]):  # matches that name a point with the skip bit, on either side
        points1["flags"][feats1[i]], points2["flags"][feats2[i]] = (sr.POINT_SKIP, 0) if k % 2 else (0, sr.POINT_SKIP)
    return dict(kps1=kps1, points1=points1, cam1=cam1, kps2=kps2, points2=points2, cam2=cam2, match12=match12, truth=(s, R, t),
                inlier_truth=inlier_truth, good1=good1)


def solver(pair, seed, fix_scale=0, params=REFERENCE, trace=False, level_sigma2=LEVEL_SIGMA2):
    s = sr.Sim3Solver(pair["kps1"], pair["points1"], pair["cam1"], pair["kps2"], pair["points2"], pair["cam2"], pair["match12"], level_sigma2,
                      fix_scale=fix_scale, seed=seed, trace=trace)
    s.set_ransac_parameters(**params)
    return s


def run_restatement(pair, seed, fix_scale=0, params=REFERENCE, n_calls=N_CALLS, n_iterations=N_ITERATIONS, trace=False):
    """The restatement's n_calls iterate(n_iterations) on a pair -> (list of (Result, generator state behind the call), the solver)."""
    s = solver(pair, seed, fix_scale, params, trace)
    out = []
    for _ in range(n_calls):
        r = s.iterate(n_iterations)
        out.append((r, None if s.code else s.rng.s))
    return out, s


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pair, spec with every field, the restatement's calls, the traced solver), computed once per session."""
    c = dict(dict(kind="", params=REFERENCE, n_calls=N_CALLS, n_iterations=N_ITERATIONS, fix_scale=0), **CASES[name])
    pair = make_pair(c["nc"], c["outliers"], c["noise"], c["scene"], c["kind"], fix_scale=c["fix_scale"])
    want, s = run_restatement(pair, c["seed"], c["fix_scale"], c["params"], c["n_calls"], c["n_iterations"], trace=True)
    return pair, c, want, s


def standin_objects(pair, moved=True):
    """The pair as KeyFrame / MapPoint stand-ins for ORB_SLAM2::DeviceSim3Solver: every feature with a point record gets a MapPoint (bad
    where the record carries the skip bit), observed at its own slot -- but with `moved` the point of the first correspondence is observed
    at the slot of the last one (a GetIndexInKeyFrame that is not i1: the bound comes from that keypoint's octave).  -> (objects for
    host_sim3_binding.dropin, the arrays the constructor must build: keys1, points1, points2, match12)."""
    o = dict(kps1=pair["kps1"], kps2=pair["kps2"])
    cams = np.zeros(2, CAMERA)
    cams[0], cams[1] = pair["cam1"], pair["cam2"]
    o["cameras"] = cams
    for k in ("1", "2"):
        pts = pair["points" + k]
        n = len(pts)
        o["world" + k], o["bad" + k] = pts["pos"].copy(), (pts["flags"] & sr.POINT_SKIP).astype(np.uint8)
        o["index" + k], o["kf_points" + k] = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)
    m12 = pair["match12"]
    o["matched12"] = m12.copy()  # table 2 is indexed by keyframe 2's feature
    good = [i for i in range(len(m12)) if m12[i] >= 0 and not (pair["points1"]["flags"][i] & 1) and not (pair["points2"]["flags"][m12[i]] & 1)]
    keys1 = pair["kps1"].copy()
    if moved:
        a = good[0]
        b = next(i for i in reversed(good) if pair["kps1"]["octave"][i] != pair["kps1"]["octave"][a])
        o["index1"][a] = b
        keys1["octave"][a] = pair["kps1"]["octave"][b]
    points1, points2 = np.zeros(len(m12), POINT), np.zeros(len(pair["kps2"]), POINT)
    points1["flags"] = points2["flags"] = sr.POINT_SKIP
    match12 = np.full(len(m12), -1, np.int32)
    for i in good:
        points1[i], points2[m12[i]] = (pair["points1"]["pos"][i], 0), (pair["points2"]["pos"][m12[i]], 0)
        match12[i] = m12[i]
    return o, dict(keys1=keys1, points1=points1, points2=points2, match12=match12)


RESULT_FIELDS = ("code", "has_sim3", "no_more", "n_inliers", "n_correspondences", "max_iterations", "iterations", "iterations_call",
                 "best_inliers", "status")


def assert_result_equal(got, got_inlier, want, what):
    """got: an amos_sim3_result record (numpy void), got_inlier: uint8 [n1]; want: a restatement Result.  == on the bytes."""
    for f in RESULT_FIELDS:
        assert int(got[f]) == int(getattr(want, f)), f"{what}: {f} = {int(got[f])}, the restatement has {int(getattr(want, f))}"
    for f, w in (("R12", want.R12), ("t12", want.t12), ("s12", np.array([want.s12], f32)), ("T12", want.T12)):
        g = np.asarray(got[f], f32).reshape(-1)
        assert g.tobytes() == np.asarray(w, f32).tobytes(), f"{what}: {f} differs from the restatement\n{g}\n{w}"
    assert np.asarray(got_inlier, np.uint8).tobytes() == want.inlier.tobytes(), f"{what}: the inlier flags differ from the restatement"


def check_cases():
    """The seeds do what the cases are named for (run when this file is imported, and once more by tests/test_sim3_cpu.py)."""
    for name in ("three_calls", "three_calls_fix_scale"):
        _, _, want, _ = case(name)
        assert [w.has_sim3 for w, _ in want][0] == 0 and any(w.has_sim3 for w, _ in want[1:]), (name, [w.has_sim3 for w, _ in want])
    _, _, want, s = case("early_stop_in_round")
    assert want[0][0].has_sim3 and 8 < want[0][0].iterations < ROUND - 8, want[0][0].iterations
    _, _, want, s = case("two_rounds_no_success")
    w = want[0][0]
    counts = [h.n_inliers for h in s.trace]
    assert not w.has_sim3 and w.no_more and ROUND < w.iterations == w.max_iterations == len(counts) < 300
    top = [k for k, c in enumerate(counts) if c == max(counts)]
    assert len(top) >= 2 and top[0] < ROUND <= top[-1] and w.best_inliers == max(counts) <= 20, (top, max(counts))
    assert s.best is s.trace[top[-1]]  # the LAST of equal maxima stands
    _, c, want, s = case("noise_free")
    assert all(w.has_sim3 and w.n_inliers == c["nc"] and w.iterations_call == 1 for w, _ in want)
    _, _, want, _ = case("n_equals_min_inliers")
    assert want[0][0].max_iterations == 1 and want[0][0].iterations == 1 and want[0][0].no_more and not want[0][0].has_sim3
    _, c, want, _ = case("n_below_min_inliers")
    assert all(w.no_more and w.iterations == 0 and rng == c["seed"] for w, rng in want)
    _, _, want, s = case("degenerate")
    assert not want[0][0].has_sim3 and want[0][0].iterations > ROUND
    idx = [sorted(h.idx) for h in s.trace]
    assert any(len({0, 1, 2} & set(i)) >= 2 for i in idx), "no sample with two coincident points"
    assert any(set(i) <= {3, 4, 5, 6, 7, 8} for i in idx), "no collinear sample"
    _, _, want, s = case("pure_translation")
    assert all(h.degenerate and h.n_inliers == 0 for h in s.trace) and not want[0][0].has_sim3 and want[0][0].best_inliers == 0
    assert np.array_equal(s.best.R, np.eye(3, dtype=f32))


check_cases()  # at import: every user of the cases runs on seeds that do what the cases are named for (0.5 s, the results are kept)

if __name__ == "__main__":
    for name in CASES:
        _, _, want, s = case(name)
        print(name, [(w.has_sim3, w.n_inliers, w.iterations, w.best_inliers, w.no_more) for w, _ in want], "N", s.N, "maxIts", s.max_iterations)
