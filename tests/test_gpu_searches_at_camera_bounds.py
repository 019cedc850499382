"""The three projection-window point searches on the GPU at the image bounds of the reference's cameras -- TUM1 (bounds inside the image),
Bonn and EuRoC mono (outside; tests/ref_settings.py) -- where the other search tests run with (0, w, 0, h), at which x - mnMinX is exact and a
frustum test against the image rectangle cannot be told from one against the bounds.  The comparisons are the ones of
tests/test_gpu_local_points.py, tests/test_gpu_motion_model.py, tests/test_gpu_reloc_search.py and the host-form files, called from here
(their `check` / `run_device` / `restate`): device against restatement bit for bit.  The keypoints are undistorted with the camera, the grid
is built from cells computed at its bounds, and every scene moves eight points between the camera's min_x and 0 and eight left of both
rectangles (ref_settings.move_into_the_sliver).

Non-vacuity, asserted in every test: at least one point that projects finitely fails the bounds test, at least one match is accepted, and
the restatement on the same inputs with (0, w, 0, h) gives another result (another set of points in view or another d_match)."""
import numpy as np
import pytest

import local_points_restatement as lr
import motion_model_restatement as mr
import ref_settings as rs
import reloc_restatement as rr
import test_gpu_local_points as local_points
import test_gpu_motion_model as motion_model
import test_gpu_reloc_search as reloc_search

pytestmark = pytest.mark.gpu

CAMERAS = list(rs.SEARCH_CAMERAS)
ANYWHERE = (-1e30, 1e30, -1e30, 1e30)


@pytest.fixture(scope="module")
def scenes(ob, synth):
    """camera -> scene: two frames of the camera's size extracted by the oracle with the file's ORB parameters, keypoints undistorted"""
    return {name: rs.camera_scene(ob, synth, name) for name in CAMERAS}


def with_u_right(sc, lo, hi):
    """the scene with uRight > 0 on half of the features, as the searches' own scenes have it"""
    rng = np.random.default_rng(len(sc["frames"][0][0]))
    frames = [(k, d, np.where(rng.random(len(k)) < 0.5, k["x"] - rng.uniform(lo, hi, len(k)), -1).astype(np.float32)) for k, d in sc["frames"]]
    return dict(sc, frames=frames)


def sliver(sc, points, cam):
    rs.move_into_the_sliver(points, cam["Rcw"], cam["tcw"], sc["intr"], sc["bounds"], sc["image_bounds"])


@pytest.mark.parametrize("with_ur", [True, False])
@pytest.mark.parametrize("camera,th", [("TUM1", 1.0), ("Bonn", 3.0), ("EuRoC", 5.0), ("EuRoC", 1.0)])
def test_local_points(gpu_lib, scenes, camera, th, with_ur):
    sc = with_u_right(scenes[camera], 3, 30)
    cams = local_points.cameras_of(sc, th=th)
    points = local_points.scene_points(sc, cams, (700, 65), seed=int(th) + len(camera))
    for f in range(2):
        sliver(sc, points[f], cams[f])
    stats, want = local_points.check(gpu_lib, sc["frames"], points, cams, local_points.no_occupancy(sc["frames"]), sc["sf"], sc["bounds"], with_ur)
    for f, (k, d, r) in enumerate(sc["frames"]):
        w = want[f]
        image = lr.search_local_points(k, d, r if with_ur else None, points[f], cams[f], np.zeros(len(k), np.uint8), sc["sf"], sc["image_bounds"])
        flipped = int((w["in_view"] != image["in_view"]).sum())
        print(f"frame {f}: in view {w['n_in_view']} at the camera's bounds, {image['n_in_view']} at the image's, {flipped} points differ")
        assert flipped >= 1 and (w["n_in_view"] != image["n_in_view"] or not np.array_equal(w["match"], image["match"]))
        assert (w["reason"] == lr.REASONS["outside"]).sum() >= 1 and w["n_matches"] >= 1
    assert 0.3 * 700 < want[0]["n_in_view"] < 0.7 * 700 and want[0]["n_matches"] > 0.25 * want[0]["n_in_view"]
    # the host form on the same inputs
    k, d, r = sc["frames"][0]
    mt = gpu_lib.OrbMatcher()
    q, iv, m, st = mt.local_points(k, d, points[0], cams[0], np.zeros(len(k), np.uint8), sc["sf"], bounds=sc["bounds"], u_right=r if with_ur else None)
    mt.close()
    assert np.array_equal(iv, want[0]["in_view"]) and np.array_equal(m, want[0]["match"]) and tuple(st) == tuple(stats[0])


@pytest.mark.parametrize("with_ur", [True, False])
@pytest.mark.parametrize("camera,motion,th", [("TUM1", "sideways", 7.0), ("Bonn", "forward", 15.0), ("EuRoC", "backward", 7.0), ("EuRoC", "mono", 15.0)])
def test_motion_model(gpu_lib, scenes, camera, motion, th, with_ur):
    sc = with_u_right(scenes[camera], 0, 20)
    cams = motion_model.cameras_of(sc, motion, th=th)
    points = motion_model.scene_points(sc, (700, 65), seed=int(th) + len(camera) + len(motion))
    for f in range(2):
        sliver(sc, points[f], cams[f])
    stats, want = motion_model.check(gpu_lib, sc["frames"], points, cams, sc["sf"], sc["bounds"], with_ur)
    for f, (k, d, r) in enumerate(sc["frames"]):
        w = want[f]
        image = mr.search_motion_model(k, d, r if with_ur else None, points[f], cams[f], sc["sf"], sc["image_bounds"])
        anywhere = mr.project(points[f], cams[f], len(sc["sf"]), (-np.inf, np.inf, -np.inf, np.inf))[1]
        print(f"frame {f}: projected {w['n_projected']} at the camera's bounds, {image['n_projected']} at the image's, {int(anywhere.sum())} anywhere")
        assert ((anywhere == 1) & (w["projected"] == 0)).sum() >= 1 and w["n_matches"] >= 1
        assert w["n_projected"] != image["n_projected"] or not np.array_equal(w["match"], image["match"])
    assert want[0]["flags"] == want[1]["flags"] == mr.MOTION_FLAGS[motion]
    assert want[0]["n_matches"] > 30 and want[0]["pass"] == 1 and want[0]["status"] == 0
    # the host form on the same inputs
    k, d, r = sc["frames"][0]
    mt = gpu_lib.OrbMatcher()
    q, pj, m, st = mt.motion_model(k, d, points[0], cams[0], sc["sf"], bounds=sc["bounds"], u_right=r if with_ur else None)
    mt.close()
    assert np.array_equal(pj, want[0]["projected"]) and np.array_equal(m, want[0]["match"]) and tuple(st) == tuple(stats[0])


@pytest.mark.parametrize("th,orb_dist", rr.PARAMS)
@pytest.mark.parametrize("camera", CAMERAS)
def test_relocalisation(gpu_lib, scenes, camera, th, orb_dist):
    sc = scenes[camera]
    n = len(sc["frames"][1][0])
    kw = dict(th=th, orb_dist=orb_dist)
    pairs = [reloc_search.make_pair(sc, 0, n, 1, motion=0, **kw), reloc_search.make_pair(sc, 0, 300, 2, motion=1, **kw),
             reloc_search.make_pair(sc, 1, 200, 3, motion=0, **kw)]
    for p in pairs:
        sliver(sc, p["points"], p["cam"])
    out, want = reloc_search.check(gpu_lib, sc, sc["frames"], pairs)
    image = reloc_search.restate(sc["frames"], pairs, sc["sf"], sc["image_bounds"])
    anywhere = reloc_search.restate(sc["frames"], pairs, sc["sf"], ANYWHERE)
    for k, (w, im, aw) in enumerate(zip(want, image, anywhere)):
        print(f"pair {k}: projected {w['n_projected']} at the camera's bounds, {im['n_projected']} at the image's, {aw['n_projected']} anywhere")
        assert ((aw["projected"] == 1) & (w["projected"] == 0)).sum() >= 1 and w["n_matches"] >= 1
        assert w["n_projected"] != im["n_projected"] or not np.array_equal(w["match"], im["match"])
    assert want[0]["n_matches"] > 20 and want[0]["n_occupied"] > n // 4 and want[0]["n_found"] > n // 8 and want[1]["n_matches"] > 5
    # the host form on the first pair's inputs
    p, w = pairs[0], want[0]
    kps, desc = sc["frames"][0]
    mt = gpu_lib.OrbMatcher()
    query, projected, match, stats = mt.reloc(kps, desc, p["points"], p["cam"], sc["sf"], p["match_in"], found=p["found"], bounds=sc["bounds"])
    mt.close()
    assert tuple(int(stats[k]) for k in rr.STAT_FIELDS) == tuple(int(w[k]) for k in rr.STAT_FIELDS)
    assert np.array_equal(match, w["match"]) and np.array_equal(projected, w["projected"])
    assert query[w["projected"] == 1].tobytes() == w["query"][w["projected"] == 1].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the C++ drop-ins

@pytest.mark.parametrize("camera,stereo,th", [("TUM1", True, 1.0), ("Bonn", False, 3.0), ("EuRoC", True, 5.0)])
def test_search_local_points_drop_in(gpu_lib, scenes, camera, stereo, th):
    """ORB_SLAM2::SearchLocalPoints against the host chain before it (isInFrustum on the host, then ORBmatcherFor::SearchByProjection) on
    stand-in objects that carry the camera's bounds, as tests/test_gpu_local_points_host.py holds it at (0, 640, 0, 480)."""
    import host_local_binding as hl
    sc = scenes[camera]
    (k0, d0), (k1, d1) = sc["frames"]
    rng = np.random.default_rng(17)
    cam = lr.camera(*lr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1]), *sc["intr"], th=th, nn_ratio=0.8)
    pts = lr.make_points(rng, k1, d1, 700, cam, sc["sf"])
    sliver(sc, pts, cam)
    bad, seen = (rng.random(700) < 0.05).astype(np.uint8), (rng.random(700) < 0.05).astype(np.uint8)
    # the table level and the logarithm agree away from the table's entries: no tested point may have its ratio within 1e-4 of one
    ratio = pts["max_distance"].astype(np.float64) / np.linalg.norm(pts["pos"].astype(np.float64) - cam["Ow"].astype(np.float64), axis=1)
    assert not (np.abs(ratio[:, None] / sc["sf"].astype(np.float64) - 1.0) < 1e-4).any()
    ur = np.where(rng.random(len(k0)) < 0.5, k0["x"] - rng.uniform(3, 30, len(k0)), -1).astype(np.float32) if stereo else None
    occupant = np.where(rng.random(len(k0)) < 0.2, rng.integers(0, 3, len(k0)), -1).astype(np.int32)
    got = hl.search_local_points("dropin", k0, d0, ur, pts, cam, occupant, sc["sf"], sc["bounds"], bad, seen)
    want = hl.search_local_points("parent", k0, d0, ur, pts, cam, occupant, sc["sf"], sc["bounds"], bad, seen)
    iv = want["in_view"] == 1
    print(camera, got["n_matches"], want["n_matches"], int(iv.sum()))
    assert np.array_equal(got["in_view"], want["in_view"]) and 200 < iv.sum() < 500 and not iv[(bad | seen) == 1].any()
    assert got["track"][iv].tobytes() == want["track"][iv].tobytes() and np.array_equal(got["level"][iv], want["level"][iv])
    assert np.array_equal(got["visible"], want["in_view"].astype(np.int32)) and np.array_equal(want["visible"], got["visible"])
    assert np.array_equal(got["match"], want["match"]) and got["n_matches"] == want["n_matches"] > 100
    at_camera, at_image = lr.frustum(pts, cam, sc["sf"], sc["bounds"]), lr.frustum(pts, cam, sc["sf"], sc["image_bounds"])
    assert (at_camera[3] == lr.REASONS["outside"]).sum() >= 1 and (at_camera[1] != at_image[1]).sum() >= 1


@pytest.mark.parametrize("camera,motion,stereo,th", [("TUM1", "sideways", True, 7.0), ("Bonn", "forward", True, 7.0), ("EuRoC", "sideways", False, 15.0)])
def test_search_by_motion_model_drop_in(gpu_lib, scenes, camera, motion, stereo, th):
    """ORB_SLAM2::SearchByMotionModel against the chain Tracking::TrackWithMotionModel had before it and against the restatement, on stand-in
    objects that carry the camera's bounds, as tests/test_gpu_motion_model_host.py holds it at (0, 640, 0, 480)."""
    import host_motion_binding as hm
    sc = scenes[camera]
    (k0, d0), (k1, d1) = sc["frames"]
    rng = np.random.default_rng(17)
    last = mr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1])
    cam = mr.camera(*mr.moved(last, **mr.MOTIONS[motion]), *last, *sc["intr"], th=th, retry_below=20)
    assert mr.motion_flags(cam) == mr.MOTION_FLAGS[motion]
    pts = mr.make_last_points(rng, k1, d1, len(k1), last, sc["intr"], replace=False)  # index i is feature i of the last frame
    sliver(sc, pts, cam)
    ur = np.where(rng.random(len(k0)) < 0.5, k0["x"] - rng.uniform(0, 20, len(k0)), -1).astype(np.float32) if stereo else None
    got = hm.search_motion_model("dropin", k0, d0, ur, k1, pts, cam, sc["sf"], sc["bounds"], None)
    want = hm.search_motion_model("parent", k0, d0, ur, k1, pts, cam, sc["sf"], sc["bounds"], None)
    res = mr.search_motion_model(k0, d0, ur, pts, cam, sc["sf"], sc["bounds"])
    print(camera, got["n_matches"], want["n_matches"], res["n_matches"], res["pass"])
    assert got["n_matches"] == want["n_matches"] == res["n_matches"] >= 20 and np.array_equal(got["match"], want["match"])
    assert np.array_equal(got["match"], res["match"]) and res["pass"] == 1
    image = mr.search_motion_model(k0, d0, ur, pts, cam, sc["sf"], sc["image_bounds"])
    anywhere = mr.project(pts, cam, len(sc["sf"]), (-np.inf, np.inf, -np.inf, np.inf))[1]
    assert ((anywhere == 1) & (res["projected"] == 0)).sum() >= 1
    assert res["n_projected"] != image["n_projected"] or not np.array_equal(res["match"], image["match"])
