"""The host forms of the relocalisation search on the GPU: amos_match_reloc against the restatement, the drop-in
ORB_SLAM2::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) against the existing adaptor over the host class on stand-in
objects, and ORB_SLAM2::RefineRelocalization against the Python chain of restatements on three seeded candidates."""
import numpy as np
import pytest

import motion_model_restatement as mr
import reloc_restatement as rr

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def hb(gpu_lib):
    import host_binding
    host_binding.host()
    return host_binding


@pytest.fixture(scope="module")
def small(ob, synth):
    orc = ob.Oracle(500, 1.2, 4)
    frames = [orc.extract(synth.frame(3, k, 240, 320)) for k in range(2)]
    return dict(frames=frames, sf=orc.tables()["scale"], bounds=(0.0, 320.0, 0.0, 240.0), intr=(260.0, 260.0, 160.0, 120.0))


@pytest.mark.parametrize("th,orb_dist", rr.PARAMS)
def test_host_form_equals_the_restatement(gpu_lib, small, th, orb_dist):
    sc = small
    (kps, desc), (kkps, kdesc) = sc["frames"]
    mt = gpu_lib.OrbMatcher()
    for seed, m, ffm, with_found in ((1, len(kkps), 0, True), (2, 65, 1, True), (3, 200, 1, False), (4, 0, 0, False)):
        rng = np.random.default_rng(seed)
        points = rr.make_points(rng, kkps, kdesc, m, rr.KF_POSE, sc["intr"], sc["sf"])
        match_in, found = rr.entry_state(rng, len(kps), m)
        cam = rr.camera(*mr.moved(rr.KF_POSE, **rr.CUR_MOTIONS[seed % 2]), *sc["intr"], th=th, orb_dist=orb_dist, found_from_match=ffm)
        fd = found if with_found else None
        want = rr.search(kps, desc, points, cam, fd, match_in, sc["sf"], sc["bounds"])
        query, projected, match, stats = mt.reloc(kps, desc, points, cam, sc["sf"], match_in, found=fd, bounds=sc["bounds"])
        print(m, {k: (int(stats[k]), want[k]) for k in rr.STAT_FIELDS})
        assert tuple(int(stats[k]) for k in rr.STAT_FIELDS) == tuple(int(want[k]) for k in rr.STAT_FIELDS)
        assert np.array_equal(match, want["match"]) and np.array_equal(projected, want["projected"])
        pj = want["projected"] == 1
        assert query[pj].tobytes() == want["query"][pj].tobytes()
    # nothing at all, and a disabled pair
    q0, p0, m0, s0 = mt.reloc(kps[:0], desc[:0], points[:0], cam, sc["sf"], match_in[:0], bounds=sc["bounds"])
    assert len(q0) == len(p0) == len(m0) == 0 and tuple(s0) == (0,) * 8
    points = rr.make_points(np.random.default_rng(5), kkps, kdesc, 100, rr.KF_POSE, sc["intr"], sc["sf"])
    off = rr.camera(*rr.KF_POSE, *sc["intr"], enabled=0)
    _, _, m1, s1 = mt.reloc(kps, desc, points, off, sc["sf"], match_in, bounds=sc["bounds"])
    assert np.array_equal(m1, match_in) and tuple(s1) == (0,) * 7 + (1,)
    mt.close()


@pytest.fixture(scope="module")
def adaptor_scene(hb, ob, synth):
    from test_gpu_host_adaptors import Scene
    return Scene(hb, ob, synth, stream=31, seed=21)


def test_drop_in_search_equals_the_host_class(hb, adaptor_scene):
    """SearchByProjection<Frame, KeyFrame, MapPoint> == ORBmatcherFor::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) on
    the stand-in map of tests/test_gpu_host_adaptors.py, with one MapPoint* at two keyframe indices twice over: one of the two points is in
    sAlreadyFound (both of its indices are skipped), the other is not (both are searched)."""
    import host_reloc_binding as hrb
    s = adaptor_scene
    rng = np.random.default_rng(1)
    already = (rng.random(s.pts.n) < 0.1).astype(np.uint8)
    occupants = np.where(rng.random(s.n1) < 0.1, rng.integers(0, s.n0, s.n1), -1).astype(np.int32)   # CurrentFrame.mvpMapPoints on entry
    point_of0 = s.point_of0.copy()
    good = np.nonzero((point_of0 >= 0) & (s.bad[np.maximum(point_of0, 0)] == 0))[0]
    a, a2, b, b2 = good[10], good[11], good[40], good[41]
    point_of0[a2], point_of0[b2] = point_of0[a], point_of0[b]
    already[point_of0[a]], already[point_of0[b]] = 1, 0
    kf, k0 = hb.test_kf(s.cam0, s.k0, s.d0, s.ur0, point_of0)
    cur, k1 = hb.test_kf(s.cam1, s.k1, s.d1, s.ur1, occupants)
    total = 0
    for th, orb_dist, ori in ((10.0, 100, True), (3.0, 64, True), (10.0, 100, False), (3.0, 64, False)):
        want_n, want = hb.ref_search_reloc(cur, kf, s.pts, already, th, orb_dist, 0.9, ori)
        got_n, got, _ = hrb.search_reloc(cur, kf, s.pts, already, th, orb_dist, ori)
        print(th, orb_dist, ori, want_n, got_n)
        assert got_n == want_n and np.array_equal(got, want)
        assert np.array_equal(got[occupants >= 0], occupants[occupants >= 0]) and not (got == point_of0[a]).any()
        total += got_n
    assert total > 200


REFINE_CASES = {  # seed, PnP inliers, usable keyframe points, wrong matches among the inliers, points beside their feature: chosen with
    # rr.refine so that each branch of Tracking.cc:2717-2771 ends one case
    "stops_below_ten": ((1, 8, 60, 0, 0), ["optimise"], 8),
    "stops_after_the_first_search": ((2, 30, 200, 3, 0), ["optimise", "search", "optimise"], 197),
    "reaches_the_third_optimisation": ((3, 30, 60, 6, 8), ["optimise", "search", "optimise", "search", "optimise"], 52),
}


@pytest.mark.parametrize("name", list(REFINE_CASES))
def test_refine_relocalization(hb, small, name):
    import host_reloc_binding as hrb
    sc = small
    kps, desc = sc["frames"][0]
    n, sf = len(kps), sc["sf"]
    args, steps, n_good = REFINE_CASES[name]
    c = rr.refine_case(kps, desc, sc["intr"], sf, *args)
    inv_sigma2 = (f32(1.0) / (sf * sf)).astype(f32)  # what the harness fills into mvInvLevelSigma2
    want = rr.refine(kps, desc, c["kf_points"], c["ident"], c["table_pos"], c["vp_matches"], c["inliers"], c["start"], sc["intr"], sf, inv_sigma2,
                     sc["bounds"])
    assert want["steps"] == steps and want["n_good"] == n_good  # the branch the case was chosen for
    T = np.eye(4, dtype=f32)
    T[:3, :3], T[:3, 3] = np.asarray(c["start"][0], f32).reshape(3, 3), c["start"][1]
    fx, fy, cx, cy = sc["intr"]
    cam_cur = hb.test_camera(T, sf, fx, fy, cx, cy, 0.0, 0.0, bounds=sc["bounds"])
    cam_kf = hb.test_camera(np.eye(4, dtype=f32), sf, fx, fy, cx, cy, 0.0, 0.0, bounds=sc["bounds"])  # (the keyframe's pose is not read)
    pts_rec = c["kf_points"]
    obs = ((pts_rec["flags"] & rr.HAS_OBS) != 0).astype(np.int32)
    pts, keep = hb.test_points(c["table_pos"], np.zeros((n, 3), f32), pts_rec["desc"], obs, np.zeros(n, np.uint8), pts_rec["min_distance"],
                               pts_rec["max_distance"])
    kf_kps = kps.copy()
    kf_kps["angle"] = pts_rec["angle"]
    kf, keep_kf = hb.test_kf(cam_kf, kf_kps, desc, None, c["ident"])
    cur, keep_cur = hb.test_kf(cam_cur, kps, desc, None, np.full(n, -1, np.int32))
    got = hrb.refine_relocalization(cur, kf, pts, c["vp_matches"], c["inliers"])
    print(name, got["n_good"], want["n_good"], got["set_pose"], int((got["points"] >= 0).sum()))
    assert got["n_good"] == want["n_good"]
    assert np.array_equal(got["points"], want["points"]) and np.array_equal(got["outlier"], want["outlier"])
    assert got["Tcw"].tobytes() == want["Tcw"].tobytes() and got["set_pose"] == steps.count("optimise")
