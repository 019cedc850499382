"""Step 2 of Tracking::SearchLocalPoints without a GPU: the numpy restatement (tests/local_points_restatement.py) on hand cases for every
gate of isInFrustum, the table form of PredictScale against the logarithm, a seeded scene, and the new entry points in the library."""
import ctypes

import numpy as np
import pytest

import local_points_restatement as lr


@pytest.mark.parametrize("sf,nl", [(1.2, 8), (1.2, 12), (1.5, 5), (1.1, 16)])
def test_table_level_equals_the_logarithm(sf, nl):
    """level = ceil(log(ratio) / log(scaleFactor)) clamped to [0, n_levels - 1] (MapPoint.cc:571-586), except within a relative 1e-5 of a
    table entry, where the logarithm's rounding decides; that share of 10^5 log-uniform ratios stays below 0.1 %."""
    table = np.ones(nl, np.float32)
    for i in range(1, nl):
        table[i] = table[i - 1] * np.float32(sf)  # ORBextractor.cc:505-510
    rng = np.random.default_rng(5)
    ratio = np.exp(rng.uniform(np.log(0.5), np.log(float(table[-1]) * 1.5), 100000)).astype(np.float32)
    near = (np.abs(ratio[:, None].astype(np.float64) / table.astype(np.float64) - 1.0) < 1e-5).any(1)
    print(sf, nl, "left out:", near.mean())
    assert near.mean() < 1e-3
    logs = np.log(np.float32(sf))  # mfLogScaleFactor = log(mfScaleFactor), float
    want = np.clip(np.ceil(np.log(ratio) / logs), 0, nl - 1).astype(np.int32)
    got = lr.table_level(ratio, table)
    assert np.array_equal(got[~near], want[~near])
    assert lr.table_level(np.float32(np.nan), table) == 0


@pytest.fixture(scope="module")
def hand(ob):
    kps, desc = lr.hand_frame()
    out = {}
    for name, (pts, cam, *_rest) in lr.hand_cases().items():
        out[name] = lr.search_local_points(kps, desc, None, pts, cam, np.zeros(len(kps), np.uint8), lr.HAND_SCALE, lr.HAND_BOUNDS)
    return out


@pytest.mark.parametrize("name", ["behind", "nan_projection", "on_min_x_and_max_x", "distance_limits", "view_cos_limit", "radius_narrow",
                                  "radius_wide", "levels"])
def test_hand_case(hand, name):
    pts, cam, in_view, status, levels, matches = lr.hand_cases()[name]
    got = hand[name]
    assert list(got["in_view"]) == in_view and got["status"] == status and got["n_in_view"] == sum(in_view)
    if levels is not None:
        assert list(got["query"]["level"]) == levels
    if matches is not None:
        assert list(got["match"]) == matches and got["n_matches"] == sum(m >= 0 for m in matches)


def test_hand_case_values(hand):
    q = hand["on_min_x_and_max_x"]["query"]
    assert q["proj_x"][0] == 0.0 and q["proj_x"][1] == 640.0 and q["proj_y"][0] == 240.0
    assert q["proj_xr"][0] == np.float32(0.0) - np.float32(40.0)  # u - mbf * invz, invz = 1
    assert hand["view_cos_limit"]["query"]["view_cos"][0] == np.float32(0.5)
    assert float(hand["radius_narrow"]["query"]["view_cos"][0]) > 0.998 > float(hand["radius_wide"]["query"]["view_cos"][0])


def test_restatement_on_a_seeded_scene(ob, synth):
    """Every gate rejects its share, every level occurs, and the search finds most of the points in view."""
    nl = 4
    orc = ob.Oracle(500, 1.2, nl)
    k0, d0 = orc.extract(synth.frame(3, 0, 240, 320))
    k1, d1 = orc.extract(synth.frame(3, 1, 240, 320))
    sf = orc.tables()["scale"]
    bounds = (0.0, 320.0, 0.0, 240.0)
    rng = np.random.default_rng(11)
    cam = lr.camera(*lr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1]), 260.0, 260.0, 160.0, 120.0)
    pts = lr.make_points(rng, k1, d1, 700, cam, sf)
    r = lr.search_local_points(k0, d0, None, pts, cam, np.zeros(len(k0), np.uint8), sf, bounds)
    print(r["n_in_view"], r["n_matches"], np.bincount(r["query"]["level"][r["in_view"] == 1], minlength=nl))
    assert 0.3 * len(pts) < r["n_in_view"] < 0.7 * len(pts)
    assert (np.bincount(r["query"]["level"][r["in_view"] == 1], minlength=nl) > 0).all()
    assert r["n_matches"] > 0.3 * r["n_in_view"] and r["status"] == 0
    # the scene sends about 15 % of the points into each of the four gates (depth / image bounds, distance range, viewing angle) and half
    # that into the skip flag, two branches per gate where it has two: every branch rejects at least 4 %, every gate at least 10 %
    count = {name: int((r["reason"] == code).sum()) for name, code in lr.REASONS.items()}
    print(count)
    for name in ("behind", "outside", "near", "far", "skip"):
        assert count[name] >= 0.04 * len(pts), (name, count)
    for gate in (("behind", "outside"), ("near", "far"), ("angle",)):
        assert sum(count[g] for g in gate) >= 0.10 * len(pts), (gate, count)
    m = r["match"]
    assert ((m >= 0).sum() <= r["n_matches"]) and (r["in_view"][m[m >= 0]] == 1).all()


def test_library_exports_the_local_map_entry_points(pkg):
    names = ("amos_match_local_points_batch_device", "amos_match_local_points")
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in names:
        assert name in pkg.EXPORTS and hasattr(L, name), name
    assert hasattr(pkg.OrbMatcher, "local_points_batch_device") and hasattr(pkg.OrbMatcher, "local_points")
    assert (pkg.MAP_POINT_DTYPE.itemsize, pkg.LOCAL_CAMERA_DTYPE.itemsize, pkg.LOCAL_STATS_DTYPE.itemsize, pkg.MAP_QUERY_DTYPE.itemsize) == (80, 92, 16, 56)
    assert pkg.MAP_POINT_DTYPE == lr.MAP_POINT and pkg.LOCAL_CAMERA_DTYPE == lr.CAMERA
    hdr = open(pkg.LIB_PATH.replace("amos-slam_amd/csrc/libamos_frontend.so", "include/amos_frontend.h")).read()
    assert "80 bytes" in hdr and "92 bytes" in hdr
    lib = pkg.lib()  # NULL arguments are AMOS_ERR_INVALID before any device is touched
    assert lib.amos_match_local_points_batch_device(None, None) == -1
    assert lib.amos_match_local_points(None, None, None, None, 0, None, 0, None, None, None, 8, 0.0, 640.0, 0.0, 480.0, None, None, None, None) == -1
    assert b"amos_match_local_points" in lib.amos_last_error()
