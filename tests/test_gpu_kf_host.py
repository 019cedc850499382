"""GPU: the C++ drop-ins of amos-slam_amd/host/KeyFrameSearch.h -- ORB_SLAM2::SearchForTriangulation (one call for all neighbours, and its
single-pair form) and ORB_SLAM2::SearchByBoW(pKF1, pKF2, vpMatches12) -- on stand-in KeyFrame / MapPoint objects against the host class
(ORBmatcherFor::SearchForTriangulation / SearchByBoW(KF, KF) through the existing adaptors, one call per neighbour) and the CPU oracle."""
import numpy as np
import pytest

import bow_search_cases as bc
import kf_search_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk(gpu_lib):
    import host_kf_binding
    host_kf_binding.lib()
    return host_kf_binding


def _pairs_of(match12):
    i = np.nonzero(match12 >= 0)[0]
    return np.stack([i, match12[i]], 1).astype(np.int32)


@pytest.mark.parametrize("only_stereo", [0, 1])
@pytest.mark.parametrize("nodes", sorted(bc.NODE_LEVELS))
def test_search_for_triangulation(hk, ob, synth, nodes, only_stereo):
    """the LocalMapping shape: keyframe 1 against three neighbours, each with its own F12 and pose"""
    sides = kc.synth_sides(ob, synth, "small", nodes, 0.3)
    w, h = bc.SIZES["small"][:2]
    K, motions, (geos, lv) = kc.camera(w, h), kc.shift_motions(w, h), kc.synth_geometry("small")
    pairs, kinds = kc.PAIRS[:3], kc.PAIR_GEOMETRY[:3]
    k1, k2s = sides[pairs[0][0]], [sides[b] for _, b in pairs]
    poses, f12s = [hk.pose_of_neighbour(*motions[g]) for g in kinds], [geos[g]["f12"] for g in kinds]
    for ori in (0, 1):
        res = {w_: hk.triangulation(w_, k1, k2s, K, poses, f12s, lv[0], only_stereo, ori) for w_ in ("dropin", "parent", "single")}
        total = 0
        for p, (k2, g) in enumerate(zip(k2s, kinds)):
            want_n, want = kc.oracle_triangulation(k1, k2, geos[g], lv[0], lv[1], only_stereo, ori)
            assert res["parent"]["pairs"][p].tolist() == _pairs_of(want).tolist() and res["parent"]["returned"][p] == want_n
            for w_ in ("dropin", "single"):
                assert res[w_]["pairs"][p].tolist() == res["parent"]["pairs"][p].tolist(), (w_, p)
            assert res["single"]["returned"][p] == want_n
            total += want_n
        assert res["dropin"]["returned"][0] == total and (only_stereo or total >= 30)


def test_search_for_triangulation_random_pair_and_empty(hk):
    """an epipole inside the image, computed from the poses by the drop-in as by the host class; a neighbour without features"""
    k1, k2, geo, lv = kc.random_pair(5)
    K = kc.camera(640, 480)
    pose = hk.pose_of_neighbour(kc._rot(1e-3, -2e-3, 1.5e-3), [0.02, -0.01, 0.3])
    empty = kc.side(np.zeros((0, 32), np.uint8), [], {})
    a = hk.triangulation("dropin", k1, [k2, empty, k2], K, [pose] * 3, [geo["f12"]] * 3, lv[0], 0, 1)
    b = hk.triangulation("parent", k1, [k2, empty, k2], K, [pose] * 3, [geo["f12"]] * 3, lv[0], 0, 1)
    assert [p.tolist() for p in a["pairs"]] == [p.tolist() for p in b["pairs"]]
    assert len(a["pairs"][0]) >= 8 and len(a["pairs"][1]) == 0 and a["returned"][0] == b["returned"].sum()


@pytest.mark.parametrize("ori", [0, 1])
@pytest.mark.parametrize("nodes", sorted(bc.NODE_LEVELS))
def test_search_by_bow_kf(hk, ob, synth, nodes, ori):
    """vpMatches12 holds keyframe 2's map points; a bad map point is none on either side"""
    sides = kc.synth_sides(ob, synth, "small", nodes, 0.8)
    k1, k2s = sides[1], [sides[0], sides[2]]
    rng = np.random.default_rng(3)
    bad = [(k, int(i)) for k in range(3) for i in rng.choice(len(([k1] + k2s)[k]["desc"]), 40, replace=False)]
    a = hk.search_by_bow("dropin", k1, k2s, 0.75, ori, bad)
    b = hk.search_by_bow("parent", k1, k2s, 0.75, ori, bad)
    assert np.array_equal(a["match12"], b["match12"]) and a["returned"].tolist() == b["returned"].tolist()

    def without_bad(s, k):
        hp = s["has_point"].copy()
        hp[[i for kk, i in bad if kk == k]] = 0
        return dict(s, has_point=hp)
    for p, k2 in enumerate(k2s):
        want_n, want = kc.oracle_bow_kf(without_bad(k1, 0), without_bad(k2, p + 1), 0.75, ori)
        # a matched keyframe-2 feature holds a point: the drop-in's pointer identifies the feature
        assert a["match12"][p].tolist() == want.tolist() and a["returned"][p] == want_n
    assert a["returned"].min() >= 30
