"""The host forms of the loop-closing point search on the GPU: amos_match_loop_points (one query from host arrays) and the C++ drop-in
ORB_SLAM2::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (amos-slam_amd/host/KeyFrameLoopPoints.h, through tests/host_loop_points)
equal the resident call on the shared scene, and the drop-in equals the existing host class's SearchByProjection(pKF, Scw, ...)."""
import numpy as np
import pytest

import host_loop_points_binding as hlb
import loop_points_restatement as lp
from test_gpu_loop_points import Resident

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shared():
    return lp.shared()


@pytest.fixture(scope="module")
def resident_rows(gpu_lib, shared):
    """the resident call on both queries of the scene, with the entry rows as the only source of spAlreadyFound (what a vpMatched carries)"""
    sc, _ = shared
    queries = sc["queries"].copy()
    queries["found_from_match"] = 1
    r = Resident(gpu_lib, sc["kfs"], sc["bounds"], sc["capacity"])
    loop, stats, _, _ = r.run(points=sc["points"], first=sc["first"], count=sc["count"], queries=queries, rows=sc["rows"], sf=sc["sf"], maps=sc["maps"])
    r.close()
    assert stats["n_matches"][0] > 100 and stats["n_researched"][0] >= 3 and stats["accepted"].tolist() == [1, 0]
    return queries, loop, stats


def test_host_form_equals_the_resident_call(gpu_lib, shared, resident_rows):
    sc, _ = shared
    queries, loop, stats = resident_rows
    mt = gpu_lib.OrbMatcher()
    for k in range(2):
        kps, desc = sc["kfs"][k]
        a, c = int(sc["first"][k]), int(sc["count"][k])
        q = queries[k].copy()
        q["frame"] = 0
        got, st = mt.loop_points(dict(keys_un=kps, desc=desc), sc["points"][a:a + c], q, sc["sf"], matched=sc["rows"][k], point_of_feature2=sc["maps"][k],
                                 bounds=sc["bounds"])
        assert np.array_equal(got, loop[k, :len(kps)]) and st.tobytes() == stats[k].tobytes(), k
    # the bytes as the source, a keyframe without features, a list without points, a disabled query
    kps, desc = sc["kfs"][0]
    q = sc["queries"][0].copy()
    q["found_from_match"] = 0
    c = int(sc["count"][0])
    got, st = mt.loop_points(dict(keys_un=kps, desc=desc), sc["points"][:c], q, sc["sf"], matched=sc["rows"][0], found=sc["found"][:c], bounds=sc["bounds"])
    want = lp.search(kps, desc, sc["points"][:c], q, sc["rows"][0], sc["found"][:c], None, sc["sf"], sc["bounds"])
    assert np.array_equal(got, want["loop_match"]) and tuple(int(st[n]) for n in lp.STATS) == tuple(int(want[n]) for n in lp.STATS)
    got, st = mt.loop_points(dict(keys_un=kps[:0], desc=desc[:0]), sc["points"][:c], q, sc["sf"], bounds=sc["bounds"])
    assert len(got) == 0 and st["n_matches"] == 0 and st["n_in_view"] > 100 and st["skipped"] == 0
    got, st = mt.loop_points(dict(keys_un=kps, desc=desc), sc["points"][:0], q, sc["sf"], matched=sc["rows"][0], bounds=sc["bounds"])
    assert (got == -1).all() and st["n_candidates"] == 0 and st["n_total"] == int((sc["rows"][0] != -1).sum())
    q["enabled"] = 0
    got, st = mt.loop_points(dict(keys_un=kps, desc=desc), sc["points"][:c], q, sc["sf"], matched=sc["rows"][0], bounds=sc["bounds"])
    assert (got == -1).all() and st["skipped"] == 1 and st["n_total"] == 0
    mt.close()


def pointer_row(row, pf2, n_points):
    """the scene's entry row as a vpMatched: a feature whose keyframe-2 feature holds a point of the list carries that point, every other
    occupied feature a point that is not in the list"""
    out = np.full(len(row), -1, np.int32)
    for i, j in enumerate(row):
        if j == -1:
            continue
        p = int(pf2[j]) if 0 <= j < len(pf2) else -1
        out[i] = p if 0 <= p < n_points else -2
    return out


def test_dropin_equals_the_resident_call_and_the_host_class(shared, resident_rows):
    sc, _ = shared
    queries, loop, stats = resident_rows
    for k in range(2):
        kps, desc = sc["kfs"][k]
        a, c = int(sc["first"][k]), int(sc["count"][k])
        pts = sc["points"][a:a + c]
        kf, keep = hlb.standin(kps, desc, lp.INTR, sc["sf"], sc["bounds"])
        row_in = pointer_row(sc["rows"][k], sc["maps"][k], c)
        if k == 0:  # list points and points from outside the list among the entries
            assert (row_in >= 0).sum() >= 1 and (row_in == -2).sum() >= 1
        n, row_out, st, _ = hlb.search("dropin", kf, pts, queries[k]["Scw"], row_in)
        want_row = np.where(loop[k, :len(kps)] >= 0, loop[k, :len(kps)], row_in)
        assert n == stats["n_matches"][k] and np.array_equal(row_out, want_row), k
        assert st.tobytes() == stats[k].tobytes(), k
        n_ref, row_ref, _, _ = hlb.search("host_class", kf, pts, queries[k]["Scw"], row_in)
        print(f"query {k}: drop-in {n}, host class {n_ref}")
        assert n_ref == n and np.array_equal(row_ref, row_out), k
