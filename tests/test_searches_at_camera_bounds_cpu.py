"""The restatements of the three projection-window point searches against the oracle searches they are already held to
(orc_features_in_area / orc_search_by_projection_* through a frame view), at the image bounds of TUM1, Bonn and EuRoC mono instead of
(0, w, 0, h): tests/test_local_points_cpu.py, tests/test_motion_model_cpu.py and tests/test_reloc_search_cpu.py at the reference's cameras.
The comparisons are theirs: lr.search_local_points asserts its Python loop against the oracle's search by itself, the motion-model search
runs under both implementations, and the relocalisation check calls test_reloc_search_cpu.oracle_search.  Keypoints are undistorted with
the camera; every scene moves eight points between the camera's min_x and 0 and eight left of both rectangles.

Non-vacuity, asserted in every test: at least one point that projects finitely fails the bounds test, at least one match is accepted, and
the restatement on the same inputs with (0, w, 0, h) gives another result."""
import numpy as np
import pytest

import local_points_restatement as lr
import motion_model_restatement as mr
import ref_settings as rs
import reloc_restatement as rr
import test_reloc_search_cpu as reloc_cpu  # oracle_search

CAMERAS = list(rs.SEARCH_CAMERAS)


@pytest.fixture(scope="module")
def scenes(ob, synth):
    return {name: rs.camera_scene(ob, synth, name) for name in CAMERAS}


def sliver(sc, points, cam):
    rs.move_into_the_sliver(points, cam["Rcw"], cam["tcw"], sc["intr"], sc["bounds"], sc["image_bounds"])


@pytest.mark.parametrize("camera", CAMERAS)
def test_local_points_restatement(scenes, camera):
    """The seeded scene of tests/test_local_points_cpu.py: every gate rejects its share, every level occurs, most points in view match."""
    sc = scenes[camera]
    (k0, d0), (k1, d1) = sc["frames"]
    cam = lr.camera(*lr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1]), *sc["intr"])
    pts = lr.make_points(np.random.default_rng(11), k1, d1, 700, cam, sc["sf"])
    sliver(sc, pts, cam)
    free = np.zeros(len(k0), np.uint8)
    r = lr.search_local_points(k0, d0, None, pts, cam, free, sc["sf"], sc["bounds"])  # asserts Python loop == oracle search
    image = lr.search_local_points(k0, d0, None, pts, cam, free, sc["sf"], sc["image_bounds"])
    flipped = int((r["in_view"] != image["in_view"]).sum())
    print(camera, sc["bounds"], "in view", r["n_in_view"], image["n_in_view"], "flipped", flipped, "matches", r["n_matches"], image["n_matches"])
    assert 0.3 * len(pts) < r["n_in_view"] < 0.7 * len(pts) and r["n_matches"] > 0.3 * r["n_in_view"] and r["status"] == 0
    assert (np.bincount(r["query"]["level"][r["in_view"] == 1], minlength=sc["nl"]) > 0).all()
    count = {name: int((r["reason"] == code).sum()) for name, code in lr.REASONS.items()}
    for name in ("behind", "outside", "near", "far", "skip", "angle"):
        assert count[name] >= 0.04 * len(pts), (name, count)
    assert flipped >= 1 and (r["n_in_view"] != image["n_in_view"] or not np.array_equal(r["match"], image["match"]))


@pytest.mark.parametrize("camera", CAMERAS)
def test_motion_model_restatement(scenes, camera):
    """The seeded scene of tests/test_motion_model_cpu.py: the Python loop equals the oracle on a contested scene."""
    sc = scenes[camera]
    (k0, d0), (k1, d1) = sc["frames"]
    last = mr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1])
    pts = mr.make_last_points(np.random.default_rng(5), k1, d1, 400, last, sc["intr"])
    cam = mr.camera(*mr.moved(last, **mr.MOTIONS["sideways"]), *last, *sc["intr"], th=7.0, retry_below=0)
    sliver(sc, pts, cam)
    a = mr.search_motion_model(k0, d0, None, pts, cam, sc["sf"], sc["bounds"])
    b = mr.search_motion_model(k0, d0, None, pts, cam, sc["sf"], sc["bounds"], impl=mr.search_python)
    image = mr.search_motion_model(k0, d0, None, pts, cam, sc["sf"], sc["image_bounds"])
    anywhere = mr.project(pts, cam, len(sc["sf"]), (-np.inf, np.inf, -np.inf, np.inf))[1]
    print(camera, sc["bounds"], "projected", a["n_projected"], image["n_projected"], int(anywhere.sum()), "matches", a["n_matches"], image["n_matches"])
    assert np.array_equal(a["match"], b["match"]) and a["n_matches"] == b["n_matches"] > 100
    assert a["n_matches"] > (a["match"] >= 0).sum() and 300 < a["n_projected"] < 400
    assert ((anywhere == 1) & (a["projected"] == 0)).sum() >= 1
    assert a["n_projected"] != image["n_projected"] or not np.array_equal(a["match"], image["match"])


@pytest.mark.parametrize("th,orb_dist", rr.PARAMS)
@pytest.mark.parametrize("camera", CAMERAS)
def test_relocalisation_restatement(scenes, camera, th, orb_dist):
    """The check of tests/test_reloc_search_cpu.py: the restatement equals the reference-side prefilter + the oracle's loop."""
    sc = scenes[camera]
    (kps, desc), (kkps, kdesc) = sc["frames"]
    rng = np.random.default_rng(len(camera) * 100 + int(th))
    points = rr.make_points(rng, kkps, kdesc, len(kkps), rr.KF_POSE, sc["intr"], sc["sf"])
    match_in, found = rr.entry_state(rng, len(kps), len(points))
    cam = rr.camera(*mr.moved(rr.KF_POSE, **rr.CUR_MOTIONS[0]), *sc["intr"], th=th, orb_dist=orb_dist)
    sliver(sc, points, cam)
    got = rr.search(kps, desc, points, cam, found, match_in, sc["sf"], sc["bounds"])
    n, m, q, pidx = reloc_cpu.oracle_search(kps, desc, points, cam, found, match_in, sc["sf"], sc["bounds"])
    assert np.array_equal(np.nonzero(got["projected"])[0], pidx)
    for name in ("u", "v", "level", "angle", "desc"):
        assert got["query"][name][pidx].tobytes() == q[name].tobytes(), name
    assert got["n_matches"] == n > 20 and np.array_equal(got["match"], m) and got["status"] == 0
    image = rr.search(kps, desc, points, cam, found, match_in, sc["sf"], sc["image_bounds"])
    anywhere = rr.search(kps, desc, points, cam, found, match_in, sc["sf"], (-1e30, 1e30, -1e30, 1e30))["projected"]
    print(camera, "projected", got["n_projected"], image["n_projected"], int(anywhere.sum()), "matches", got["n_matches"], image["n_matches"])
    assert ((anywhere == 1) & (got["projected"] == 0)).sum() >= 1
    assert got["n_projected"] != image["n_projected"] or not np.array_equal(got["match"], image["match"])
