"""SearchByBoW(KeyFrame, Frame) when the FRAME side carries a has_point array of its own: only the keyframe's features need a map point
(ORBmatcher.cc:264-270), the frame's array is never read.  One hand case in the form of bow_search_cases.hand_cases, held to the oracle on
the CPU and run on the GPU through the checks of test_gpu_bow_search.py in the batch and the host form, and the host form's staging of a
frame view with has_point beside a keyframe view without."""
import ctypes as C

import numpy as np
import pytest

import bow_restatement as br
import bow_search_cases as bc
import test_gpu_bow_search as tb


def frame_without_points():
    """(kf, f, nn_ratio, check_orientation, expected matches_f, expected n_matches): a keyframe of two features with has_point [1, 1], a
    frame of two features whose own has_point is [0, 0], all in one shared node.  Distances 3 and 5 to distinct frame features, the other
    candidate far (97 and 105); the second query finds its second best taken and searches its list again."""
    kf = bc.side([bc._first(3), bc._first(105)], [0, 0], {5: [0, 1]}, [1, 1])
    f = bc.side([bc._first(0), bc._first(100)], [0, 0], {5: [0, 1]}, [0, 0])
    return kf, f, 0.7, 0, [0, 1], 2


def host_form_with_frame_points(pkg, mt, kf, f, nn_ratio, ori):
    """amos_match_bow with BOTH views carrying their side's has_point (OrbMatcher.bow passes the keyframe's only) -> (matches_f, stats)"""
    kf, f = bc.with_csr(kf), bc.with_csr(f)
    vk, keep_k = mt._bow_view(kf["keys"], kf["desc"], kf["node_ids"], kf["node_off"], kf["node_idx"], kf.get("has_point"))
    vf, keep_f = mt._bow_view(f["keys"], f["desc"], f["node_ids"], f["node_off"], f["node_idx"], f.get("has_point"))
    matches, stats = np.full(vf.n, -1, np.int32), np.zeros(1, pkg.BOW_SEARCH_STATS_DTYPE)
    rc = mt.L.amos_match_bow(mt.h, C.byref(vk), C.byref(vf), nn_ratio, int(ori), matches.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return matches, stats[0]


def test_the_oracle_ignores_the_frames_has_point(ob):
    kf, f, nn_ratio, ori, want, want_n = frame_without_points()
    oracle_n, oracle = bc.oracle_search(ob, kf, f, nn_ratio, ori)
    assert oracle.tolist() == want and oracle_n == want_n == 2  # the expectation written in the case is the oracle's: both match
    replay, rs = br.search_by_bow(kf, f, nn_ratio, ori)
    assert replay.tolist() == want and rs == {"n_queries": 2, "n_matches": 2, "n_researched": 1}


@pytest.mark.gpu
def test_hand_case_frame_without_points(gpu_lib, ob):
    """as test_gpu_bow_search.test_hand_cases runs its cases; pack() copies the frame's zeros into its slot, so the device sees them"""
    kf, f, nn_ratio, ori, want, want_n = frame_without_points()
    oracle_n, oracle = bc.oracle_search(ob, kf, f, nn_ratio, ori)
    assert oracle.tolist() == want and oracle_n == want_n
    tb.check_pairs(gpu_lib, ob, [kf, f], [(0, 1)], nn_ratio, ori, True)
    _, rs = br.search_by_bow(kf, f, nn_ratio, ori)
    mt = gpu_lib.OrbMatcher()
    results = [mt.bow(bc.with_csr(kf), bc.with_csr(f), nn_ratio, ori),             # the host form, the keyframe's has_point only
               host_form_with_frame_points(gpu_lib, mt, kf, f, nn_ratio, ori)]     # and with the frame's own array in its view
    mt.close()
    for got, stats in results:
        assert got.tolist() == want and tuple(int(stats[k]) for k in tb.STAT_FIELDS) == tuple(rs[k] for k in tb.STAT_FIELDS) and stats["status"] == 0


@pytest.mark.gpu
def test_host_form_ignores_the_frame_views_has_point(gpu_lib, ob, synth):
    """a frame view that carries has_point while the keyframe view has none: every keyframe feature has a point, as without the array"""
    sides = bc.synth_sides(ob, synth, "small", "10")
    kf, f = dict(sides[0], has_point=None), sides[1]
    assert f["has_point"] is not None and not f["has_point"].all()
    mt = gpu_lib.OrbMatcher()
    got, stats = host_form_with_frame_points(gpu_lib, mt, kf, f, 0.7, 1)
    plain, plain_stats = mt.bow(bc.with_csr(kf), bc.with_csr(f), 0.7, 1)
    mt.close()
    want_n, want = bc.oracle_search(ob, kf, f, 0.7, 1)
    assert got.tolist() == plain.tolist() == want.tolist() and stats.tobytes() == plain_stats.tobytes() and stats["n_matches"] == want_n
