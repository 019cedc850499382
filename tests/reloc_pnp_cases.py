"""tests/reloc_pnp_cases.py -- the synthetic pairs (lost frame, candidate keyframe) of the relocalisation PnP tests, shared by
tests/test_reloc_pnp_cpu.py (host-compiled solver), tests/test_gpu_reloc_pnp.py (kernel) and tests/test_gpu_reloc_pnp_host.py (drop-in):
a frame's keypoints, the candidate's point list and a sparse SearchByBoW row whose correspondences are a pnp_restatement.scene, and the
restatement's three iterate(5) calls on it, computed once per case."""
import functools

import numpy as np

import pnp_restatement as pr
import reloc_pnp_restatement as rp

CAPACITY = 256
LEVEL_SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], np.float32)
OCTAVES = (0, 2)        # two octaves, two thresholds
REFERENCE = dict(probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991)  # Tracking.cc:2665
N_CALLS, N_ITERATIONS = 3, 5
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
POINT = np.dtype([("pos", "<f4", (3,)), ("angle", "<f4"), ("min_distance", "<f4"), ("max_distance", "<f4"), ("flags", "<i4"),
                  ("desc", "u1", (32,)), ("pad", "u1", (4,))])

# name: (correspondences, outlier fraction, pixel noise, kind)
CASES = {
    "n0": (0, 0.3, 0.5, ""), "n3": (3, 0.3, 0.5, ""), "n9": (9, 0.3, 0.5, ""), "n10": (10, 0.3, 0.5, ""), "n15": (15, 0.3, 0.5, ""),
    "n19": (19, 0.3, 0.5, ""), "n20": (20, 0.3, 0.5, ""), "n63": (63, 0.3, 0.5, ""), "n64": (64, 0.3, 0.5, ""), "n65": (65, 0.3, 0.5, ""),
    "n200": (200, 0.3, 0.5, ""),
    "clean40": (40, 0.0, 0.0, ""), "clean64_out30": (64, 0.3, 0.0, ""), "out70": (40, 0.7, 0.5, ""), "all_outliers": (40, 1.0, 0.5, ""),
    "coplanar": (40, 0.3, 0.5, "planar"), "duplicates": (14, 0.0, 0.5, "duplicates"),
    "duplicates_outliers": (14, 1.0, 0.5, "duplicates"),  # nothing qualifies, so every call runs its iterations: some samples are degenerate
    "refine_fails": (20, 0.5, 0.5, ""),  # as many inliers as minInliers: iterations qualify, Refine's strict test fails
}


def make_pair(nc, outlier_frac, noise, kind="", seed=0, n_features=None, skipped=4, K=pr.K_TUM):
    """-> dict(kps, bow_match, points, K): nc correspondences among n_features features (ascending feature order is a random order of the
    scene's points), `skipped` more matches that name points with the skip bit, the rest of the row -1."""
    rng = np.random.default_rng(1000 + seed)
    n = nc + skipped + 26 if n_features is None else n_features
    n_points = n + 10
    obj, img, _, _ = pr.scene(rng, max(nc, 1), outlier_frac, noise, planar=kind == "planar", K=K)
    obj, img = obj[:nc].copy(), img[:nc].copy()
    if kind == "duplicates" and nc >= 6:
        obj[1:6] = obj[0]
        img[1:6] = img[0]
    kps = np.zeros(n, KP)
    kps["x"], kps["y"] = rng.uniform(0, 640, n).astype(np.float32), rng.uniform(0, 480, n).astype(np.float32)
    kps["octave"] = rng.choice(OCTAVES, n)
    points = np.zeros(n_points, POINT)
    points["pos"] = rng.uniform(-3, 3, (n_points, 3)).astype(np.float32)
    points["flags"] = 2
    feats = np.sort(rng.choice(n, nc + skipped, replace=False))
    names = rng.choice(n_points, nc + skipped, replace=False)
    is_skip = np.zeros(nc + skipped, bool)
    is_skip[rng.choice(nc + skipped, skipped, replace=False)] = True
    bow = np.full(n, -1, np.int32)
    bow[feats] = names
    points["flags"][names[is_skip]] |= rp.POINT_SKIP
    good = feats[~is_skip]
    kps["x"][good], kps["y"][good] = img[:, 0], img[:, 1]
    points["pos"][names[~is_skip]] = obj
    return dict(kps=kps, bow_match=bow, points=points, K=K)


def run_restatement(pair, seed, params=REFERENCE, n_calls=N_CALLS, n_iterations=N_ITERATIONS):
    """The restatement's n_calls iterate(n_iterations) on a pair -> list of (Result, generator state behind the call)."""
    s = rp.PnPsolver(pair["kps"], pair["bow_match"], pair["points"], LEVEL_SIGMA2, pair["K"], seed)
    s.set_ransac_parameters(**params)
    out = []
    for _ in range(n_calls):
        r = s.iterate(n_iterations)
        out.append((r, None if s.code else s.rng.s))
    return out


# (scene, generator) chosen so that later calls meet the failed Refine's best set again, and so that two of the 21 samples are degenerate
FIXED_SEEDS = {"refine_fails": (40, 123), "duplicates_outliers": (50, 201)}


def case_seed(name):
    if name in FIXED_SEEDS:
        return FIXED_SEEDS[name][1]
    return 0x9E3779B97F4A7C15 ^ (sorted(CASES).index(name) * 0x100000001B3)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pair, seed, the restatement's calls), computed once per session."""
    nc, frac, noise, kind = CASES[name]
    pair = make_pair(nc, frac, noise, kind, seed=FIXED_SEEDS[name][0] if name in FIXED_SEEDS else sorted(CASES).index(name))
    seed = case_seed(name)
    return pair, seed, run_restatement(pair, seed)


RESULT_FIELDS = ("code", "has_pose", "no_more", "refined", "n_inliers", "n_correspondences", "min_inliers", "max_iterations", "iterations",
                 "iterations_call", "best_inliers", "status")


def assert_result_equal(got, got_inlier, want, what):
    """got: an amos_reloc_pnp_result record (numpy void or ctypes structure), got_inlier: uint8 [n]; want: a restatement Result."""
    for f in RESULT_FIELDS:
        g = int(got[f]) if isinstance(got, np.void) else int(getattr(got, f))
        assert g == int(getattr(want, f)), f"{what}: {f} = {g}, the restatement has {int(getattr(want, f))}"
    tcw = np.asarray(got["Tcw"] if isinstance(got, np.void) else list(got.Tcw), np.float32)
    assert tcw.tobytes() == want.Tcw.tobytes(), f"{what}: Tcw differs from the restatement\n{tcw}\n{want.Tcw}"
    assert np.asarray(got_inlier, np.uint8).tobytes() == want.inlier.tobytes(), f"{what}: the inlier flags differ from the restatement"
