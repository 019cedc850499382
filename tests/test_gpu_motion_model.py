"""amos_match_motion_model_batch_device / amos_match_motion_model on the GPU against the numpy restatement + CPU oracle
(tests/motion_model_restatement.py), bit for bit: every field of d_query where projected, d_projected, d_match with its padding, and every
stat."""
import numpy as np
import pytest

import local_points_restatement as lr  # grid_cells
import motion_model_restatement as mr

pytestmark = pytest.mark.gpu

SIZES = {"small": (320, 240, 500, 4, 260.0), "large": (640, 480, 1000, 8, 520.0)}  # width, height, features, levels, focal length
LAST_POSES = [mr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1]), mr.pose(-0.015, 0.01, -0.01, [-0.03, 0.04, -0.05])]


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
            ur = np.where(rng.random(len(kps)) < 0.5, kps["x"] - rng.uniform(0, 20, len(kps)), -1).astype(np.float32)
            frames.append((kps, desc, ur))
        out[name] = dict(frames=frames, sf=orc.tables()["scale"], bounds=(0.0, float(w), 0.0, float(h)), nl=nl,
                         intr=(focal, focal, w / 2.0, h / 2.0))
    return out


def cameras_of(scene, motion="sideways", th=7.0, retry_below=0, check_orientation=1, motions=None):
    """one camera per frame: the frame's last pose moved by `motion` (or by motions[f])"""
    cams = []
    for f, last in enumerate(LAST_POSES):
        kw = mr.MOTIONS[motion] if motions is None else motions[f]
        cur = mr.moved(last, **kw)
        cams.append(mr.camera(*cur, *last, *scene["intr"], th=th, retry_below=retry_below, mono=int(motion == "mono"),
                              check_orientation=check_orientation))
    return cams


def scene_points(scene, counts, seed):
    """frame f gets counts[f] last-frame points made from the OTHER frame's keypoints, drawn with replacement"""
    rng = np.random.default_rng(seed)
    frames = scene["frames"]
    return [mr.make_last_points(rng, frames[1 - f][0], frames[1 - f][1], counts[f], LAST_POSES[f], scene["intr"]) for f in range(len(counts))]


def run_device(pkg, frames, points, cams, sf, bounds, with_ur, pad=5):
    """One amos_match_motion_model_batch_device call on uploaded arrays -> (query, projected, match [frames][cap], stats, point_off)."""
    import torch
    nf = len(frames)
    cap = max(max(len(k) for k, _, _ in frames), 1) + pad
    kps, desc = np.zeros((nf, cap), pkg.KP_DTYPE), np.zeros((nf, cap, 32), np.uint8)
    ur, cell = np.full((nf, cap), -1, np.float32), np.full((nf, cap), -1, np.int32)
    counts = np.zeros(nf, np.int32)
    for f, (k, d, r) in enumerate(frames):
        n = len(k)
        counts[f] = n
        kps[f, :n], desc[f, :n], ur[f, :n] = k, d, r
        cell[f, :n] = lr.grid_cells(k, bounds)
    off = np.concatenate([[0], np.cumsum([len(p) for p in points])]).astype(np.int32)
    allp = np.concatenate(points) if off[-1] else np.zeros(1, mr.LAST_POINT)
    total = max(int(off[-1]), 1)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_kps, d_desc, d_ur, d_cell, d_counts, d_pts = (up(a) for a in (kps, desc, ur, cell, counts, allp))
    d_start = torch.zeros((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_items = torch.full((nf, cap), -1, dtype=torch.int32, device="cuda")
    d_query = torch.full((total, 56), 0xEE, dtype=torch.uint8, device="cuda")
    d_projected = torch.full((total,), 7, dtype=torch.uint8, device="cuda")
    d_match = torch.full((nf, cap), 12345, dtype=torch.int32, device="cuda")  # the call itself resets it
    d_stats = torch.full((nf, 8), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mt = pkg.OrbMatcher()
    mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), nf, cap, d_start.data_ptr(), d_items.data_ptr())
    mt.motion_model_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(),
                                 d_pts.data_ptr(), off, np.array(cams, mr.CAMERA), cap, sf, d_query.data_ptr(), d_projected.data_ptr(),
                                 d_match.data_ptr(), d_stats.data_ptr(), bounds=bounds, d_u_right=d_ur.data_ptr() if with_ur else None)
    mt.sync()
    torch.cuda.synchronize()
    query = np.frombuffer(d_query.cpu().numpy().tobytes(), pkg.PROJ_QUERY_DTYPE)
    stats = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.MOTION_STATS_DTYPE)
    mt.close()
    return query, d_projected.cpu().numpy(), d_match.cpu().numpy(), stats, off


STAT_FIELDS = ("n_projected", "n_matches", "n_first", "pass", "flags", "status")


def check(pkg, frames, points, cams, sf, bounds, with_ur):
    """device == restatement for every frame of the call; returns (device stats, restatement results)"""
    query, projected, match, stats, off = run_device(pkg, frames, points, cams, sf, bounds, with_ur)
    want = []
    for f, (k, d, r) in enumerate(frames):
        w = mr.search_motion_model(k, d, r if with_ur else None, points[f], cams[f], sf, bounds)
        want.append(w)
        a, b = off[f], off[f + 1]
        print(f"frame {f}: {b - a} points, projected {w['n_projected']} / {stats['n_projected'][f]}, matches {w['n_matches']} / "
              f"{stats['n_matches'][f]}, first {w['n_first']} / {stats['n_first'][f]}, pass {w['pass']} / {stats['pass'][f]}, flags {w['flags']} / "
              f"{stats['flags'][f]}, researched {stats['n_researched'][f]}")
        assert np.array_equal(projected[a:b], w["projected"]), f
        pj = w["projected"] == 1
        for name in ("u", "v", "invz", "octave", "angle", "has_obs", "desc"):
            assert query[name][a:b][pj].tobytes() == w["query"][name][pj].tobytes(), (f, name)
        assert np.array_equal(match[f, :len(k)], w["match"]), f
        assert (match[f, len(k):] == -1).all()
        assert tuple(int(stats[name][f]) for name in STAT_FIELDS) == tuple(int(w[name]) for name in STAT_FIELDS), f
        assert stats["pad"][f] == 0 and stats["n_researched"][f] >= 0
        assert stats["n_researched"][f] == mr.researched(k, d, r if with_ur else None, cams[f], sf, bounds, w), f
    return stats, want


@pytest.mark.parametrize("with_ur", [True, False])
@pytest.mark.parametrize("th", [7.0, 15.0])
@pytest.mark.parametrize("motion", ["sideways", "forward", "backward", "mono"])
@pytest.mark.parametrize("size", ["small", "large"])
def test_two_frames_against_the_restatement(gpu_lib, scenes, size, motion, th, with_ur):
    sc = scenes[size]
    cams = cameras_of(sc, motion, th=th)
    points = scene_points(sc, (700, 65), seed=int(th) + len(size) + len(motion))
    stats, want = check(gpu_lib, sc["frames"], points, cams, sc["sf"], sc["bounds"], with_ur)
    assert want[0]["flags"] == want[1]["flags"] == mr.MOTION_FLAGS[motion]
    assert want[0]["n_matches"] > 30 and want[0]["pass"] == 1 and want[0]["status"] == 0
    assert want[0]["n_matches"] > (want[0]["match"] >= 0).sum()  # contested features are counted once per accepting point
    if motion == "sideways":
        assert stats["n_researched"][0] > 0                     # 700 points drawn from fewer keypoints: both best features taken


@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("counts", [(0, 1), (63, 64), (65, 0)])
def test_small_point_counts(gpu_lib, scenes, size, counts):
    sc = scenes[size]
    points = scene_points(sc, counts, seed=sum(counts))
    check(gpu_lib, sc["frames"], points, cameras_of(sc), sc["sf"], sc["bounds"], True)
    check(gpu_lib, sc["frames"], points, cameras_of(sc, retry_below=20), sc["sf"], sc["bounds"], True)


def test_a_frame_without_keypoints(gpu_lib, scenes):
    sc = scenes["small"]
    points = scene_points(sc, (200, 200), seed=2)
    k, d, r = sc["frames"][0]
    frames = [(k[:0], d[:0], r[:0]), sc["frames"][1]]  # frame 0 has no feature at all
    stats, want = check(gpu_lib, frames, points, cameras_of(sc, retry_below=20), sc["sf"], sc["bounds"], True)
    assert stats["n_matches"][0] == 0 and stats["n_projected"][0] > 100 and stats["pass"][0] == 2
    assert stats["n_matches"][1] > 30 and stats["pass"][1] == 1


def test_check_orientation(gpu_lib, scenes):
    sc = scenes["large"]
    points = scene_points(sc, (700, 300), seed=4)
    on, _ = check(gpu_lib, sc["frames"], points, cameras_of(sc, check_orientation=1), sc["sf"], sc["bounds"], False)
    off, _ = check(gpu_lib, sc["frames"], points, cameras_of(sc, check_orientation=0), sc["sf"], sc["bounds"], False)
    assert (off["n_matches"] >= on["n_matches"]).all() and off["n_matches"][0] > on["n_matches"][0]


RETRY_MOTIONS = [dict(ry=24.0 / 520.0), mr.MOTIONS["sideways"]]  # frame 0: a yaw that moves every projection about 24 px


def test_second_search(gpu_lib, scenes):
    """One call: frame 0 finds fewer than 20 matches at th = 7 and searches again with 14, frame 1 keeps its first result."""
    sc = scenes["large"]
    cams = cameras_of(sc, th=7.0, retry_below=20, motions=RETRY_MOTIONS)
    points = scene_points(sc, (400, 400), seed=5)
    stats, want = check(gpu_lib, sc["frames"], points, cams, sc["sf"], sc["bounds"], True)
    assert want[0]["n_first"] < 20 <= want[0]["n_matches"] and want[1]["n_first"] >= 20
    assert tuple(stats["pass"]) == (2, 1) and stats["n_first"][1] == stats["n_matches"][1]
    never = cameras_of(sc, th=7.0, retry_below=0, motions=RETRY_MOTIONS)
    s0, w0 = check(gpu_lib, sc["frames"], points, never, sc["sf"], sc["bounds"], True)
    assert tuple(s0["pass"]) == (1, 1) and s0["n_matches"][0] == want[0]["n_first"]


def test_hand_cases(gpu_lib):
    """Hand cases of tests/test_motion_model_cpu.py as points of one batch, one case per frame: an identity pose projects a point at depth 1
    onto (fx X + cx, fy Y + cy), so each record of the CPU cases becomes a last-frame point."""
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    angles = np.zeros(54, np.float32)
    angles[11] = 4.0
    kps, desc = mr.hand_frame(angles)

    def point(feature, angle=0.0, has_obs=0, du=0.0):
        p = np.zeros(1, mr.LAST_POINT)
        p["pos"] = [(kps["x"][feature] + du - 320.0) / 512.0, (kps["y"][feature] - 240.0) / 512.0, 1.0]
        p["angle"], p["flags"], p["desc"] = angle, mr.HAS_OBS if has_obs else 0, desc[feature]
        return p
    fill = [point(f, has_obs=1) for f in range(20, 30)]
    cases = {
        "overwritten_last_writer_wins_bin": ([point(0, 96.0), point(0, 0.0)] + fill, 0, (11, -1)),
        "overwritten_both_lose": ([point(0, 96.0), point(0, 180.0)] + fill + [point(30, has_obs=1)], 0, (11, -1)),
        "bin_thirty": ([point(11, 2.0), point(12, 350.0)] + fill + [point(30, has_obs=1)], 0, (12, 0)),
        "second_search": ([point(f, has_obs=1) for f in range(19)] + [point(f, has_obs=1, du=10.0) for f in range(30, 36)], 20, (25, 0)),
        "first_search_stands": ([point(f, has_obs=1) for f in range(20)] + [point(f, has_obs=1, du=10.0) for f in range(30, 36)], 20, (20, 0)),
    }
    frames = [(kps, desc, np.full(len(kps), -1, np.float32))] * len(cases)
    points = [np.concatenate(c[0]) for c in cases.values()]
    cams = [mr.camera(eye, zero, eye, zero, 512.0, 512.0, 320.0, 240.0, th=7.0, retry_below=c[1]) for c in cases.values()]
    stats, want = check(gpu_lib, frames, points, cams, mr.HAND_SCALE, mr.HAND_BOUNDS, False)
    for f, (name, (_, _, (n_matches, first_feature))) in enumerate(cases.items()):
        assert want[f]["n_matches"] == n_matches and want[f]["match"][11 if name == "bin_thirty" else 0] == first_feature, name
    assert tuple(stats["pass"]) == (1, 1, 1, 2, 1)


@pytest.mark.parametrize("with_ur", [True, False])
def test_host_form_equals_the_batch_form(gpu_lib, scenes, with_ur):
    sc = scenes["large"]
    cams = cameras_of(sc, th=7.0, retry_below=20, motions=RETRY_MOTIONS)
    points = scene_points(sc, (400, 65), seed=6)
    query, projected, match, stats, off = run_device(gpu_lib, sc["frames"], points, cams, sc["sf"], sc["bounds"], with_ur)
    mt = gpu_lib.OrbMatcher()
    for f in range(2):
        k, d, r = sc["frames"][f]
        q, pj, m, st = mt.motion_model(k, d, points[f], cams[f], sc["sf"], bounds=sc["bounds"], u_right=r if with_ur else None)
        a, b = off[f], off[f + 1]
        assert np.array_equal(pj, projected[a:b]) and np.array_equal(m, match[f, :len(k)])
        assert q[pj == 1].tobytes() == query[a:b][pj == 1].tobytes()
        assert tuple(st) == tuple(stats[f])
    if with_ur:  # (without the right gate the first search finds 20 by itself)
        assert stats["pass"][0] == 2 and stats["n_matches"][0] >= 20
    k, d, r = sc["frames"][0]
    q0, pj0, m0, st0 = mt.motion_model(k[:0], d[:0], points[0][:0], cams[0], sc["sf"], bounds=sc["bounds"])  # nothing at all
    assert len(q0) == len(pj0) == len(m0) == 0 and (st0["n_projected"], st0["n_matches"], st0["n_first"], st0["pass"]) == (0, 0, 0, 2)
    mt.close()


def test_batch_of_one_equals_the_frame_inside_a_batch_of_two(gpu_lib, scenes):
    sc = scenes["small"]
    cams = cameras_of(sc, th=15.0, retry_below=20)
    points = scene_points(sc, (300, 500), seed=7)
    q2, p2, m2, s2, off = run_device(gpu_lib, sc["frames"], points, cams, sc["sf"], sc["bounds"], True)
    for f in range(2):
        q1, p1, m1, s1, _ = run_device(gpu_lib, sc["frames"][f:f + 1], points[f:f + 1], cams[f:f + 1], sc["sf"], sc["bounds"], True)
        a, b = off[f], off[f + 1]
        n = len(sc["frames"][f][0])
        assert np.array_equal(p1, p2[a:b]) and q1[p1 == 1].tobytes() == q2[a:b][p1 == 1].tobytes()
        assert np.array_equal(m1[0, :n], m2[f, :n]) and tuple(s1[0]) == tuple(s2[f])


@pytest.mark.parametrize("with_ur", [True, False])
@pytest.mark.parametrize("motion", ["sideways", "forward", "backward"])
def test_the_window_search_rebuilds_the_match(gpu_lib, scenes, motion, with_ur):
    """Across the search families: with no observations and no orientation check nothing is ever taken, so d_match is a pure function of the
    prepass.  amos_match_window_best2_batch_device on the same projections, its query frame built from the points (keypoint i carries point
    i's octave and descriptor), gives the records, and the last point in list order whose best is feature i within TH_HIGH is d_match[i]."""
    import torch
    sc = scenes["small"]
    (k, d, r), sf, bounds = sc["frames"][0], sc["sf"], sc["bounds"]
    cam = cameras_of(sc, motion, th=7.0, check_orientation=0)[0]
    points = scene_points(sc, (300, 0), seed=11)[0]
    points["flags"] &= ~mr.HAS_OBS
    query, projected, match, stats, _ = run_device(gpu_lib, [(k, d, r)], [points], [cam], sf, bounds, with_ur)
    assert stats["n_researched"][0] == 0 and stats["flags"][0] == mr.MOTION_FLAGS[motion] and stats["n_matches"][0] > 30
    n, m = len(k), len(points)
    cap = max(n, m) + 5
    kps, desc = np.zeros((2, cap), gpu_lib.KP_DTYPE), np.zeros((2, cap, 32), np.uint8)  # frame 0: the current frame, frame 1: the points
    ur, cell = np.full((2, cap), -1, np.float32), np.full((2, cap), -1, np.int32)
    kps[0, :n], desc[0, :n], ur[0, :n], cell[0, :n] = k, d, r, lr.grid_cells(k, bounds)
    kps["octave"][1, :m], desc[1, :m] = points["octave"], points["desc"]
    uv, invz = np.zeros((1, cap, 2), np.float32), np.zeros((1, cap), np.float32)
    uv[0, :m, 0], uv[0, :m, 1], invz[0, :m] = query["u"], query["v"], query["invz"]

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_kps, d_desc, d_ur, d_cell, d_uv, d_invz = (up(a) for a in (kps, desc, ur, cell, uv, invz))
    d_counts, d_pq, d_pt = up(np.array([n, m], np.int32)), up(np.array([1], np.int32)), up(np.array([0], np.int32))
    d_start = torch.zeros((2, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_items = torch.full((2, cap), -1, dtype=torch.int32, device="cuda")
    d_out = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mt = gpu_lib.OrbMatcher()
    mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), 2, cap, d_start.data_ptr(), d_items.data_ptr())
    mt.window_best2_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), d_pq.data_ptr(),
                                 d_pt.data_ptr(), 1, cap, sf, float(cam["th"]), d_out.data_ptr(), mode={0: 0, mr.FORWARD: 1, mr.BACKWARD: 2}[int(stats["flags"][0])],
                                 bounds=bounds, d_query_uv=d_uv.data_ptr(), d_query_invz=d_invz.data_ptr(),
                                 d_u_right=d_ur.data_ptr() if with_ur else None, mbf=float(cam["mbf"]))
    mt.sync()
    best2 = d_out.cpu().numpy()[:m]  # best_idx, best_dist, second_idx, second_dist
    mt.close()
    rebuilt = np.full(n, -1, np.int32)
    for i in np.nonzero(projected)[0]:
        if best2[i, 0] >= 0 and best2[i, 1] <= mr.TH_HIGH:
            rebuilt[best2[i, 0]] = i
    assert np.array_equal(rebuilt, match[0, :n])
