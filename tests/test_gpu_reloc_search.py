"""amos_match_reloc_batch_device on the GPU against the plain-Python restatement (tests/reloc_restatement.py), bit for bit: every field of
d_query where projected, d_projected, the whole d_match row with its padding, and every stat; the d_pose path; and the chain pose
optimisation -> search -> pose optimisation on resident arrays."""
import numpy as np
import pytest

import local_points_restatement as lr  # grid_cells
import motion_model_restatement as mr
import pose_optimization_cases as pc
import pose_optimization_restatement as pr
import reloc_restatement as rr

pytestmark = pytest.mark.gpu

SIZES = {"small": (320, 240, 500, 4, 260.0), "large": (640, 480, 1000, 8, 520.0)}  # width, height, features, levels, focal length
PAD_MATCH = -77  # what the padding of a d_match row holds on entry (below -1: free, and never written)
f32 = np.float32


@pytest.fixture(scope="module")
def scenes(ob, synth):
    """Two frames of the synth stream per size, extracted once by the CPU oracle; the resident arrays are uploaded from these."""
    out = {}
    for name, (w, h, nf, nl, focal) in SIZES.items():
        orc = ob.Oracle(nf, 1.2, nl)
        frames = [orc.extract(synth.frame(3, k, h, w)) for k in range(2)]
        out[name] = dict(frames=frames, sf=orc.tables()["scale"], bounds=(0.0, float(w), 0.0, float(h)), intr=(focal, focal, w / 2.0, h / 2.0))
    return out


def make_pair(sc, frame, n_points, seed, motion=0, replace=False, found=True, **cam_kw):
    """A pair on `frame`: n_points points made from the OTHER frame's keypoints (the candidate keyframe, standing at rr.KF_POSE), the current
    pose moved from it by rr.CUR_MOTIONS[motion], a third of the features set on entry and a fifth of the points found."""
    rng = np.random.default_rng(seed)
    kkps, kdesc = sc["frames"][1 - frame]
    points = rr.make_points(rng, kkps, kdesc, n_points, rr.KF_POSE, sc["intr"], sc["sf"], replace=replace)
    match_in, fd = rr.entry_state(rng, len(sc["frames"][frame][0]), n_points)
    cam = rr.camera(*mr.moved(rr.KF_POSE, **rr.CUR_MOTIONS[motion]), *sc["intr"], **cam_kw)
    return dict(frame=frame, points=points, cam=cam, found=fd if found else None, match_in=match_in)


def run_device(pkg, frames, pairs, sf, bounds, pad=5, matcher=None, repeat=1, poses=None):
    """`repeat` amos_match_reloc_batch_device calls on uploaded arrays -> [(query, projected, match [pairs][cap], stats)], point_off"""
    import torch
    nf, npairs = len(frames), len(pairs)
    cap = max(max(len(k) for k, _ in frames), 1) + pad
    kps, desc = np.zeros((nf, cap), pkg.KP_DTYPE), np.zeros((nf, cap, 32), np.uint8)
    cell, counts = np.full((nf, cap), -1, np.int32), np.zeros(nf, np.int32)
    for f, (k, d) in enumerate(frames):
        n = len(k)
        counts[f] = n
        kps[f, :n], desc[f, :n], cell[f, :n] = k, d, lr.grid_cells(k, bounds)
    off = np.concatenate([[0], np.cumsum([len(p["points"]) for p in pairs])]).astype(np.int32)
    total = max(int(off[-1]), 1)
    allp, found = np.zeros(total, rr.POINT), np.zeros(total, np.uint8)
    match = np.full((npairs, cap), PAD_MATCH, np.int32)
    for k, p in enumerate(pairs):
        allp[off[k]:off[k + 1]] = p["points"]
        if p["found"] is not None:
            found[off[k]:off[k + 1]] = p["found"]
        match[k, :len(p["match_in"])] = p["match_in"]
    with_found = any(p["found"] is not None for p in pairs)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_kps, d_desc, d_cell, d_counts, d_pts, d_found = (up(a) for a in (kps, desc, cell, counts, allp, found))
    d_pose = None if poses is None else up(np.ascontiguousarray(poses, pkg.POSE_RESULT_DTYPE))
    d_start = torch.zeros((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_items = torch.full((nf, cap), -1, dtype=torch.int32, device="cuda")
    mt = matcher or pkg.OrbMatcher()
    mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), nf, cap, d_start.data_ptr(), d_items.data_ptr())
    out = []
    for _ in range(repeat):
        d_match = up(match)
        d_query = torch.full((total, 48), 0xEE, dtype=torch.uint8, device="cuda")
        d_projected = torch.full((total,), 7, dtype=torch.uint8, device="cuda")
        d_stats = torch.full((npairs, 8), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        mt.reloc_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), nf, d_pts.data_ptr(),
                              [p["frame"] for p in pairs], off, np.array([p["cam"] for p in pairs], rr.CAMERA), cap, sf, d_query.data_ptr(),
                              d_projected.data_ptr(), d_match.data_ptr(), d_stats.data_ptr(), bounds=bounds,
                              d_found=d_found.data_ptr() if with_found else None, d_pose=None if d_pose is None else d_pose.data_ptr())
        mt.sync()
        torch.cuda.synchronize()
        out.append((np.frombuffer(d_query.cpu().numpy().tobytes(), pkg.KF_QUERY_DTYPE), d_projected.cpu().numpy(),
                    np.frombuffer(d_match.cpu().numpy().tobytes(), np.int32).reshape(npairs, cap),
                    np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.RELOC_STATS_DTYPE)))
    if matcher is None:
        mt.close()
    return out, off


def restate(frames, pairs, sf, bounds, poses=None):
    out = []
    for k, p in enumerate(pairs):
        kps, desc = frames[p["frame"]]
        pose = None if poses is None else (poses["Tcw"][k], poses["Ow"][k])
        out.append(rr.search(kps, desc, p["points"], p["cam"], p["found"], p["match_in"], sf, bounds, pose=pose))
    return out


def assert_call(got, off, frames, pairs, want):
    """every pair of one device call equals its restatement"""
    query, projected, match, stats = got
    for k, (p, w) in enumerate(zip(pairs, want)):
        a, b = off[k], off[k + 1]
        n = len(frames[p["frame"]][0])
        print(f"pair {k}: frame {p['frame']}, {b - a} points:", {name: (int(stats[name][k]), int(w[name])) for name in rr.STAT_FIELDS})
        assert tuple(int(stats[name][k]) for name in rr.STAT_FIELDS) == tuple(int(w[name]) for name in rr.STAT_FIELDS), k
        assert np.array_equal(match[k, :n], w["match"]), k
        assert (match[k, n:] == PAD_MATCH).all(), k
        if w["skipped"]:  # nothing of the pair is written
            assert (projected[a:b] == 7).all() and (query[a:b].view(np.uint8) == 0xEE).all(), k
            continue
        assert np.array_equal(projected[a:b], w["projected"]), k
        pj = w["projected"] == 1
        for name in ("u", "v", "level", "angle", "desc"):
            assert query[name][a:b][pj].tobytes() == w["query"][name][pj].tobytes(), (k, name)


def check(pkg, sc, frames, pairs, **kw):
    out, off = run_device(pkg, frames, pairs, sc["sf"], sc["bounds"], **kw)
    want = restate(frames, pairs, sc["sf"], sc["bounds"], kw.get("poses"))
    for got in out:
        assert_call(got, off, frames, pairs, want)
    return out, want


@pytest.mark.parametrize("check_ori", [1, 0])
@pytest.mark.parametrize("th,orb_dist", rr.PARAMS)
@pytest.mark.parametrize("size", ["small", "large"])
def test_three_pairs_over_two_frames(gpu_lib, scenes, size, th, orb_dist, check_ori):
    """Pairs 0 and 1 share frame 0 with different poses, points and entry matches; pair 2 searches frame 1."""
    sc = scenes[size]
    n = SIZES[size][2]
    kw = dict(th=th, orb_dist=orb_dist, check_orientation=check_ori)
    pairs = [make_pair(sc, 0, n, 1, motion=0, **kw), make_pair(sc, 0, 300, 2, motion=1, **kw), make_pair(sc, 1, 200, 3, motion=0, **kw)]
    out, want = check(gpu_lib, sc, sc["frames"], pairs)
    assert want[0]["n_matches"] > 20 and want[0]["n_occupied"] > n // 4 and want[0]["n_found"] > n // 8 and want[1]["n_matches"] > 5
    assert not np.array_equal(want[0]["match"], want[1]["match"])


@pytest.mark.parametrize("size", ["small", "large"])
def test_point_counts_at_the_wave_boundary(gpu_lib, scenes, size):
    """130, 1 and 0 points (two pairs on frame 0), then 64 and 65."""
    sc = scenes[size]
    check(gpu_lib, sc, sc["frames"], [make_pair(sc, 0, 130, 4), make_pair(sc, 0, 1, 5, motion=1), make_pair(sc, 1, 0, 6)])
    check(gpu_lib, sc, sc["frames"], [make_pair(sc, 1, 64, 7), make_pair(sc, 0, 65, 8, motion=1)])


@pytest.mark.parametrize("size", ["small", "large"])
def test_contended_features(gpu_lib, scenes, size):
    """Points drawn with replacement at four times the feature count: many points find both features of their entry record taken."""
    sc = scenes[size]
    n = SIZES[size][2]
    pairs = [make_pair(sc, 0, 4 * n, 9, replace=True, th=10.0, orb_dist=100)]
    want = restate(sc["frames"], pairs, sc["sf"], sc["bounds"])
    assert want[0]["n_researched"] > 0  # on the CPU side of the same inputs: the case exercises wave_research
    out, _ = check(gpu_lib, sc, sc["frames"], pairs)
    assert out[0][3]["n_researched"][0] == want[0]["n_researched"] > 0


def test_a_frame_without_features(gpu_lib, scenes):
    sc = scenes["small"]
    k, d = sc["frames"][0]
    frames = [(k[:0], d[:0]), sc["frames"][1]]
    pairs = [make_pair(sc, 0, 200, 10), make_pair(sc, 1, 200, 11)]
    pairs[0]["match_in"] = pairs[0]["match_in"][:0]
    out, want = check(gpu_lib, sc, frames, pairs)
    assert want[0]["n_matches"] == 0 and want[0]["n_projected"] > 50 and want[0]["n_occupied"] == 0 and want[1]["n_matches"] > 5


def test_a_disabled_pair(gpu_lib, scenes):
    sc = scenes["small"]
    pairs = [make_pair(sc, 0, 300, 12), make_pair(sc, 0, 300, 13, motion=1, enabled=0), make_pair(sc, 1, 100, 14, found_from_match=1)]
    out, want = check(gpu_lib, sc, sc["frames"], pairs)
    (query, projected, match, stats), = out
    n = len(sc["frames"][0][0])
    assert np.array_equal(match[1, :n], pairs[1]["match_in"]) and stats["skipped"][1] == 1 and tuple(stats[1])[:7] == (0,) * 7
    assert stats["skipped"][0] == 0 and stats["n_matches"][0] > 5


def test_found_from_match(gpu_lib, scenes):
    """With and without d_found beside it; the matches on entry name a third of the features' points."""
    sc = scenes["large"]
    for found in (True, False):
        pairs = [make_pair(sc, 0, 1000, 15, found=found, found_from_match=1), make_pair(sc, 0, 400, 16, motion=1, found=found, found_from_match=0)]
        out, want = check(gpu_lib, sc, sc["frames"], pairs)
        plain = rr.search(*sc["frames"][0], pairs[0]["points"], rr.camera(*mr.moved(rr.KF_POSE, **rr.CUR_MOTIONS[0]), *sc["intr"]),
                          pairs[0]["found"], pairs[0]["match_in"], sc["sf"], sc["bounds"])
        assert want[0]["n_found"] > plain["n_found"] + 100 and want[0]["n_candidates"] < plain["n_candidates"]


def test_the_same_handle_twice(gpu_lib, scenes):
    sc = scenes["large"]
    mt = gpu_lib.OrbMatcher()
    pairs = [make_pair(sc, 0, 1000, 17), make_pair(sc, 1, 500, 18, motion=1, found_from_match=1)]
    (first, second), _ = check(gpu_lib, sc, sc["frames"], pairs, matcher=mt, repeat=2)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    small = scenes["small"]
    check(gpu_lib, small, small["frames"], [make_pair(small, 0, 65, 19)], matcher=mt)  # a smaller call on the grown scratch
    mt.close()


def pose_records(pkg, cams):
    """amos_pose_result records that hold the cameras' poses as a pose optimisation would have stored them"""
    poses = np.zeros(len(cams), pkg.POSE_RESULT_DTYPE)
    for k, c in enumerate(cams):
        Rt = [float(v) for v in c["Rcw"]] + [float(v) for v in c["tcw"]]
        poses["Rt"][k] = Rt
        poses["Tcw"][k], poses["Ow"][k] = pr.pose_store(Rt)
    return poses


@pytest.mark.parametrize("size", ["small", "large"])
def test_the_pose_from_the_device(gpu_lib, scenes, size):
    """d_pose holds the same floats as the cameras: the result equals the host-camera path's; the cameras' own poses are not read."""
    sc = scenes[size]
    n = SIZES[size][2]
    pairs = [make_pair(sc, 0, n, 20, motion=0), make_pair(sc, 0, 300, 21, motion=1), make_pair(sc, 1, 65, 22, motion=1)]
    (host,), off = run_device(gpu_lib, sc["frames"], pairs, sc["sf"], sc["bounds"])
    poses = pose_records(gpu_lib, [p["cam"] for p in pairs])
    for k, p in enumerate(pairs):
        assert poses["Tcw"][k].reshape(3, 4)[:, :3].tobytes() == p["cam"]["Rcw"].tobytes()
        assert poses["Ow"][k].tobytes() == rr.camera_centre(p["cam"]["Rcw"], p["cam"]["tcw"]).tobytes()
    blind = [dict(p, cam=p["cam"].copy()) for p in pairs]
    for p in blind:
        p["cam"]["Rcw"], p["cam"]["tcw"] = np.eye(3, dtype=f32).reshape(9), [9.0, 9.0, 9.0]
    (dev,), _ = check(gpu_lib, sc, sc["frames"], blind, poses=poses)
    assert np.array_equal(dev[1], host[1]) and np.array_equal(dev[2], host[2]) and dev[3].tobytes() == host[3].tobytes()
    pj = host[1] == 1
    assert dev[0][pj].tobytes() == host[0][pj].tobytes() and host[3]["n_matches"][0] > 20


def test_chain_pose_search_pose(gpu_lib, scenes):
    """PoseOptimization (clear_outliers = 1) -> the search with d_pose and found_from_match -> PoseOptimization on resident arrays, nothing
    returns to the host in between; equal to pose_optimization_restatement -> reloc_restatement -> pose_optimization_restatement.  The
    points are frame 0's own features back-projected through the true pose; 120 features are matched on entry (SearchByBoW's part), ten
    of them to a wrong point; the start pose is perturbed from the truth.  (The pose kernel takes its start pose from the host camera, so
    both optimisations start from the same one.)"""
    import torch
    pkg = gpu_lib
    sc = scenes["small"]
    kps, desc = sc["frames"][0]
    n, sf, bounds, intr = len(kps), sc["sf"], sc["bounds"], sc["intr"]
    rng = np.random.default_rng(23)
    points = rr.make_points(rng, kps, desc, n, rr.KF_POSE, intr, sf, skip_share=0.0, behind=False)
    match_in = np.full(n, -1, np.int32)
    edges = rng.permutation(n)[:120]
    match_in[edges] = edges
    match_in[edges[:10]] = rng.integers(0, n, 10)
    Rs, ts = mr.moved(rr.KF_POSE, rx=0.004, ry=-0.003, rz=0.002, t=(0.01, -0.008, 0.006))
    start = pc.camera(Rs, ts, *intr, 20.0)
    inv_sigma2 = (f32(1.0) / (sf * sf)).astype(f32)
    rcam = rr.camera(Rs, ts, *intr, th=10.0, orb_dist=100, found_from_match=1)
    has_obs = (points["flags"] & rr.HAS_OBS) != 0
    fill = 7
    r1, o1, m1 = pr.pose_optimization(kps, None, match_in, points["pos"], has_obs, start, inv_sigma2, np.full(n, fill, np.uint8), 1)
    s = rr.search(kps, desc, points, rcam, None, m1, sf, bounds, pose=(r1["Tcw"], r1["Ow"]))
    r2, o2, m2 = pr.pose_optimization(kps, None, s["match"], points["pos"], has_obs, start, inv_sigma2, o1, 1)
    print("edges", r1["n_edges"], "inliers", r1["n_inliers"], "additional", s["n_matches"], "edges", r2["n_edges"], "inliers", r2["n_inliers"])
    assert r1["n_edges"] == 120 and 100 <= r1["n_inliers"] < 120 and s["n_matches"] > 50 and r2["n_inliers"] > r1["n_inliers"] + 50

    cap = n + 5
    k2, d2, cell = np.zeros((1, cap), pkg.KP_DTYPE), np.zeros((1, cap, 32), np.uint8), np.full((1, cap), -1, np.int32)
    k2[0, :n], d2[0, :n], cell[0, :n] = kps, desc, lr.grid_cells(kps, bounds)
    mrow = np.full((1, cap), -1, np.int32)
    mrow[0, :n] = match_in

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_kps, d_desc, d_cell, d_counts, d_pts, d_match = up(k2), up(d2), up(cell), up(np.array([n], np.int32)), up(points), up(mrow)
    d_start = torch.zeros((1, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_items = torch.full((1, cap), -1, dtype=torch.int32, device="cuda")
    d_query = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
    d_projected = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    d_outlier = torch.full((1, cap), fill, dtype=torch.uint8, device="cuda")
    d_res1 = torch.zeros((1, pkg.POSE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_res2 = torch.zeros((1, pkg.POSE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    off = np.array([0, n], np.int32)
    flags_offset = pkg.RELOC_POINT_DTYPE.fields["flags"][1]
    mt = pkg.OrbMatcher()
    mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), 1, cap, d_start.data_ptr(), d_items.data_ptr())
    pose_args = dict(point_stride=64, flags_offset=flags_offset, has_obs_bit=pkg.RELOC_POINT_HAS_OBS, clear_outliers=True)
    mt.pose_optimization_batch_device(d_kps.data_ptr(), d_counts.data_ptr(), d_match.data_ptr(), d_pts.data_ptr(), off,
                                      np.array([start], pkg.POSE_CAMERA_DTYPE), cap, inv_sigma2, d_outlier.data_ptr(), d_res1.data_ptr(), **pose_args)
    mt.reloc_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), 1, d_pts.data_ptr(), [0],
                          off, np.array([rcam], rr.CAMERA), cap, sf, d_query.data_ptr(), d_projected.data_ptr(), d_match.data_ptr(),
                          d_stats.data_ptr(), bounds=bounds, d_pose=d_res1.data_ptr())
    mt.pose_optimization_batch_device(d_kps.data_ptr(), d_counts.data_ptr(), d_match.data_ptr(), d_pts.data_ptr(), off,
                                      np.array([start], pkg.POSE_CAMERA_DTYPE), cap, inv_sigma2, d_outlier.data_ptr(), d_res2.data_ptr(), **pose_args)
    mt.sync()
    torch.cuda.synchronize()
    res1, res2 = (np.frombuffer(d.cpu().numpy().tobytes(), pkg.POSE_RESULT_DTYPE)[0] for d in (d_res1, d_res2))
    stats = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.RELOC_STATS_DTYPE)[0]
    match, outlier, projected = d_match.cpu().numpy().view(np.int32).reshape(1, cap)[0], d_outlier.cpu().numpy()[0], d_projected.cpu().numpy()
    mt.close()
    for got, want in ((res1, r1), (res2, r2)):
        for field in ("Rt", "Tcw", "Ow", "lambda", "chi2"):
            assert pc.same_bits(got[field], want[field]), field
        for field in ("n_edges", "n_inliers", "n_inliers_with_obs", "rounds", "status", "iterations", "trials"):
            assert np.array_equal(got[field], want[field]), field
    assert tuple(int(stats[k]) for k in rr.STAT_FIELDS) == tuple(int(s[k]) for k in rr.STAT_FIELDS)
    assert np.array_equal(projected, s["projected"])
    assert np.array_equal(match[:n], m2) and (match[n:] == -1).all()
    assert np.array_equal(outlier[:n], o2) and (outlier[n:] == fill).all()
