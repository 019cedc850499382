"""amos_match_local_points_batch_device / amos_match_local_points on the GPU against the numpy restatement + CPU oracle
(tests/local_points_restatement.py), bit for bit: every field of d_query where in view, d_in_view, d_match and every stat."""
import numpy as np
import pytest

import local_points_restatement as lr

pytestmark = pytest.mark.gpu

SIZES = {"small": (320, 240, 500, 4, 260.0), "large": (640, 480, 1000, 8, 520.0)}  # width, height, features, levels, focal length


@pytest.fixture(scope="module")
def scenes(ob, synth):
    """Two frames of the synth stream per size, extracted once by the CPU oracle (the resident arrays are uploaded from these), with uRight > 0
    on half of the features."""
    out = {}
    for name, (w, h, nf, nl, focal) in SIZES.items():
        orc = ob.Oracle(nf, 1.2, nl)
        rng = np.random.default_rng(w)
        frames = []
        for k in range(2):
            kps, desc = orc.extract(synth.frame(3, k, h, w))
            ur = np.where(rng.random(len(kps)) < 0.5, kps["x"] - rng.uniform(3, 30, len(kps)), -1).astype(np.float32)
            frames.append((kps, desc, ur))
        out[name] = dict(frames=frames, sf=orc.tables()["scale"], bounds=(0.0, float(w), 0.0, float(h)), nl=nl,
                         intr=(focal, focal, w / 2.0, h / 2.0))
    return out


def cameras_of(scene, th=1.0, nn_ratio=0.8):
    poses = [lr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1]), lr.pose(-0.015, 0.01, -0.01, [-0.03, 0.04, -0.05])]
    return [lr.camera(R, t, *scene["intr"], th=th, nn_ratio=nn_ratio) for R, t in poses]


def scene_points(scene, cams, counts, seed):
    """frame f gets counts[f] points made from the OTHER frame's keypoints"""
    rng = np.random.default_rng(seed)
    frames = scene["frames"]
    return [lr.make_points(rng, frames[1 - f][0], frames[1 - f][1], counts[f], cams[f], scene["sf"]) for f in range(len(counts))]


def run_device(pkg, frames, points, cams, occupied, sf, bounds, with_ur, pad=5):
    """One amos_match_local_points_batch_device call on uploaded arrays -> (query, in_view, match [frames][cap], stats, point_off)."""
    import torch
    nf = len(frames)
    cap = max(max(len(k) for k, _, _ in frames), 1) + pad
    kps, desc = np.zeros((nf, cap), pkg.KP_DTYPE), np.zeros((nf, cap, 32), np.uint8)
    ur, cell, occ = np.full((nf, cap), -1, np.float32), np.full((nf, cap), -1, np.int32), np.zeros((nf, cap), np.uint8)
    counts = np.zeros(nf, np.int32)
    for f, (k, d, r) in enumerate(frames):
        n = len(k)
        counts[f] = n
        kps[f, :n], desc[f, :n], ur[f, :n], occ[f, :n] = k, d, r, occupied[f]
        cell[f, :n] = lr.grid_cells(k, bounds)
    off = np.concatenate([[0], np.cumsum([len(p) for p in points])]).astype(np.int32)
    allp = np.concatenate(points) if off[-1] else np.zeros(1, lr.MAP_POINT)
    total = max(int(off[-1]), 1)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_kps, d_desc, d_ur, d_cell, d_occ, d_counts, d_pts = (up(a) for a in (kps, desc, ur, cell, occ, counts, allp))
    d_start = torch.zeros((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_items = torch.full((nf, cap), -1, dtype=torch.int32, device="cuda")
    d_query = torch.full((total, 56), 0xEE, dtype=torch.uint8, device="cuda")
    d_in_view = torch.full((total,), 7, dtype=torch.uint8, device="cuda")
    d_match = torch.full((nf, cap), 12345, dtype=torch.int32, device="cuda")  # the call itself resets it
    d_stats = torch.full((nf, 4), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mt = pkg.OrbMatcher()
    mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), nf, cap, d_start.data_ptr(), d_items.data_ptr())
    mt.local_points_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(),
                                 d_pts.data_ptr(), off, np.array(cams, lr.CAMERA), d_occ.data_ptr(), cap, sf, d_query.data_ptr(),
                                 d_in_view.data_ptr(), d_match.data_ptr(), d_stats.data_ptr(), bounds=bounds,
                                 d_u_right=d_ur.data_ptr() if with_ur else None)
    mt.sync()
    torch.cuda.synchronize()
    query = np.frombuffer(d_query.cpu().numpy().tobytes(), pkg.MAP_QUERY_DTYPE)
    stats = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.LOCAL_STATS_DTYPE)
    mt.close()
    return query, d_in_view.cpu().numpy(), d_match.cpu().numpy(), stats, off


def check(pkg, frames, points, cams, occupied, sf, bounds, with_ur):
    """device == restatement for every frame of the call; returns (device stats, restatement results)"""
    query, in_view, match, stats, off = run_device(pkg, frames, points, cams, occupied, sf, bounds, with_ur)
    want = []
    for f, (k, d, r) in enumerate(frames):
        w = lr.search_local_points(k, d, r if with_ur else None, points[f], cams[f], occupied[f], sf, bounds)
        want.append(w)
        a, b = off[f], off[f + 1]
        print(f"frame {f}: {b - a} points, in view {w['n_in_view']} / {stats['n_in_view'][f]}, matches {w['n_matches']} / {stats['n_matches'][f]}, "
              f"researched {w['n_researched']} / {stats['n_researched'][f]}")
        assert np.array_equal(in_view[a:b], w["in_view"]), f
        iv = w["in_view"] == 1
        for name in ("proj_x", "proj_y", "proj_xr", "view_cos", "level", "has_obs", "desc"):
            assert query[name][a:b][iv].tobytes() == w["query"][name][iv].tobytes(), (f, name)
        assert np.array_equal(match[f, :len(k)], w["match"]), f
        assert (match[f, len(k):] == -1).all()
        assert (stats["n_in_view"][f], stats["n_matches"][f], stats["status"][f]) == (w["n_in_view"], w["n_matches"], w["status"]), f
        assert stats["n_researched"][f] == w["n_researched"], f
    return stats, want


def no_occupancy(frames):
    return [np.zeros(len(k), np.uint8) for k, _, _ in frames]


@pytest.mark.parametrize("with_ur", [True, False])
@pytest.mark.parametrize("size,th", [("small", 1.0), ("small", 3.0), ("small", 5.0), ("large", 1.0), ("large", 3.0), ("large", 5.0)])
def test_two_frames_against_the_restatement(gpu_lib, scenes, size, th, with_ur):
    sc = scenes[size]
    cams = cameras_of(sc, th=th)
    points = scene_points(sc, cams, (700, 65), seed=int(th) + len(size))
    stats, want = check(gpu_lib, sc["frames"], points, cams, no_occupancy(sc["frames"]), sc["sf"], sc["bounds"], with_ur)
    w = want[0]
    levels = np.bincount(w["query"]["level"][w["in_view"] == 1], minlength=sc["nl"])
    assert (levels > 0).all(), levels                                   # every level 0 .. L - 1 occurs
    assert 0.3 * 700 < w["n_in_view"] < 0.7 * 700 and w["n_matches"] > 0.25 * w["n_in_view"]
    assert stats["n_researched"][0] > 0                                 # 700 points drawn from fewer keypoints: conflicts occur by themselves


@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("counts", [(0, 1), (63, 64), (65, 0)])
def test_small_point_counts(gpu_lib, scenes, size, counts):
    sc = scenes[size]
    cams = cameras_of(sc)
    points = scene_points(sc, cams, counts, seed=sum(counts))
    check(gpu_lib, sc["frames"], points, cams, no_occupancy(sc["frames"]), sc["sf"], sc["bounds"], True)


def test_nn_ratio(gpu_lib, scenes):
    sc = scenes["large"]
    loose, strict = cameras_of(sc, th=3.0, nn_ratio=0.8), cameras_of(sc, th=3.0, nn_ratio=0.6)
    points = scene_points(sc, loose, (700, 300), seed=4)
    a, _ = check(gpu_lib, sc["frames"], points, loose, no_occupancy(sc["frames"]), sc["sf"], sc["bounds"], False)
    b, _ = check(gpu_lib, sc["frames"], points, strict, no_occupancy(sc["frames"]), sc["sf"], sc["bounds"], False)
    assert b["n_matches"][0] < a["n_matches"][0]


def _in_view_subset(sc, cams, n, seed):
    """n points of frame 0 that are in view and find a match on their own"""
    pts = scene_points(sc, cams, (700, 0), seed=seed)[0]
    k, d, r = sc["frames"][0]
    w = lr.search_local_points(k, d, None, pts, cams[0], np.zeros(len(k), np.uint8), sc["sf"], sc["bounds"])
    matched = np.unique(w["match"][w["match"] >= 0])
    assert len(matched) >= n
    return pts[matched[:n]]


@pytest.mark.parametrize("has_obs", [1, 0])
def test_duplicated_points(gpu_lib, scenes, has_obs):
    """Each of 50 matching points twice: with observations the second copy finds its best feature taken and searches again; without,
    nothing is ever taken, the copies overwrite each other and no window is searched twice."""
    sc = scenes["large"]
    cams = cameras_of(sc)
    base = _in_view_subset(sc, cams, 50, seed=21)
    base["flags"] = lr.HAS_OBS if has_obs else 0
    points = [np.concatenate([base, base]), base[:1]]
    stats, want = check(gpu_lib, sc["frames"], points, cams, no_occupancy(sc["frames"]), sc["sf"], sc["bounds"], False)
    if has_obs:
        assert stats["n_researched"][0] > 0
    else:
        assert stats["n_researched"][0] == 0 and stats["n_researched"][1] == 0
        m = want[0]["match"]
        assert (m[m >= 0] >= 50).sum() >= 40 and stats["n_matches"][0] > (m >= 0).sum()  # the second copies overwrote the first


def test_occupied_features(gpu_lib, scenes):
    sc = scenes["large"]
    cams = cameras_of(sc, th=3.0)
    points = scene_points(sc, cams, (700, 129), seed=8)
    rng = np.random.default_rng(3)
    occupied = [(rng.random(len(k)) < 1 / 3).astype(np.uint8) for k, _, _ in sc["frames"]]
    stats, want = check(gpu_lib, sc["frames"], points, cams, occupied, sc["sf"], sc["bounds"], True)
    for f in range(2):
        m = want[f]["match"]
        assert (occupied[f][m >= 0] == 0).all() and (m >= 0).sum() > 20


def test_empty_grid_and_all_points_skipped(gpu_lib, scenes):
    sc = scenes["small"]
    cams = cameras_of(sc)
    points = scene_points(sc, cams, (200, 200), seed=2)
    points[1]["flags"] |= lr.SKIP
    k, d, r = sc["frames"][0]
    frames = [(k[:0], d[:0], r[:0]), sc["frames"][1]]  # frame 0 has no feature at all
    stats, want = check(gpu_lib, frames, points, cams, no_occupancy(frames), sc["sf"], sc["bounds"], True)
    assert stats["n_matches"][0] == 0 and stats["n_in_view"][0] > 50
    assert tuple(stats[1]) == (0, 0, 0, 0) and (want[1]["match"] == -1).all()


def test_hand_cases(gpu_lib):
    """The hand cases of tests/test_local_points_cpu.py as one batch, one case per frame."""
    kps, desc = lr.hand_frame()
    cases = lr.hand_cases()
    frames = [(kps, desc, np.full(len(kps), -1, np.float32))] * len(cases)
    points = [c[0] for c in cases.values()]
    cams = [c[1] for c in cases.values()]
    stats, want = check(gpu_lib, frames, points, cams, no_occupancy(frames), lr.HAND_SCALE, lr.HAND_BOUNDS, False)
    for f, (name, (_, _, in_view, status, levels, matches)) in enumerate(cases.items()):
        assert list(want[f]["in_view"]) == in_view and stats["status"][f] == status, name


def test_a_complement_is_no_second_best(gpu_lib):
    """One point in view, two level-0 features inside its window: one 40 bits from the point's descriptor, one its bitwise complement, at
    distance 256.  Both loops of the reference start at 256 with strict <, so the complement is never the second best, bestLevel2 stays -1
    and the ratio test does not apply: the match stands although 40 > 0.1 * 256."""
    kps = np.zeros(2, gpu_lib.KP_DTYPE)
    kps["x"], kps["y"], kps["size"], kps["octave"] = [321.0, 319.0], [240.0, 240.0], 31.0, 0
    point = np.zeros(1, lr.MAP_POINT)
    point["pos"], point["normal"], point["max_distance"], point["flags"] = [0, 0, 2.0], [0, 0, 1.0], 1.9, lr.HAS_OBS
    point["desc"] = np.random.default_rng(40).integers(0, 256, 32, dtype=np.uint8)
    desc = np.stack([point["desc"][0], ~point["desc"][0]])
    desc[0, :5] ^= 0xFF  # 40 bits
    cam = lr.camera(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 512.0, 512.0, 320.0, 240.0, nn_ratio=0.1)
    frames = [(kps, desc, np.full(2, -1, np.float32))]
    stats, want = check(gpu_lib, frames, [point], [cam], no_occupancy(frames), lr.HAND_SCALE, lr.HAND_BOUNDS, False)
    assert list(want[0]["in_view"]) == [1] and list(want[0]["match"]) == [0, -1] and stats["n_matches"][0] == 1


@pytest.mark.parametrize("with_ur", [True, False])
def test_host_form_equals_the_batch_form(gpu_lib, scenes, with_ur):
    sc = scenes["large"]
    cams = cameras_of(sc, th=3.0)
    points = scene_points(sc, cams, (700, 65), seed=6)
    rng = np.random.default_rng(9)
    occupied = [(rng.random(len(k)) < 0.2).astype(np.uint8) for k, _, _ in sc["frames"]]
    query, in_view, match, stats, off = run_device(gpu_lib, sc["frames"], points, cams, occupied, sc["sf"], sc["bounds"], with_ur)
    k, d, r = sc["frames"][0]
    mt = gpu_lib.OrbMatcher()
    q, iv, m, st = mt.local_points(k, d, points[0], cams[0], occupied[0], sc["sf"], bounds=sc["bounds"], u_right=r if with_ur else None)
    assert np.array_equal(iv, in_view[:700]) and np.array_equal(m, match[0, :len(k)])
    assert q[iv == 1].tobytes() == query[:700][iv == 1].tobytes()
    assert tuple(st) == tuple(stats[0]) and st["n_matches"] > 100
    q0, iv0, m0, st0 = mt.local_points(k[:0], d[:0], points[0][:0], cams[0], occupied[0][:0], sc["sf"], bounds=sc["bounds"])  # nothing at all
    assert len(q0) == len(iv0) == len(m0) == 0 and tuple(st0) == (0, 0, 0, 0)
    mt.close()
