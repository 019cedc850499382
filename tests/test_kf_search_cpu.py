"""No GPU: the plain-Python replays of SearchForTriangulation and SearchByBoW(KF, KF) (tests/kf_search_restatement.py) against the CPU oracle
(orc_search_for_triangulation, orc_search_by_bow_kf) on every input the GPU tests use, the hand cases' written expectations, what the
inputs must exercise, the exports of the library and the argument checks of the host forms."""
import ctypes as C

import numpy as np
import pytest

import bow_search_cases as bc
import kf_search_cases as kc
import kf_search_restatement as kr


def _tri(k1, k2, geo, lv, only_stereo, ori):
    """the replay, held to the oracle -> its stats"""
    want_n, want = kc.oracle_triangulation(k1, k2, geo, lv[0], lv[1], only_stereo, ori)
    got, st = kr.search_for_triangulation(k1, k2, geo["f12"], geo["ex"], geo["ey"], lv[0], lv[1], only_stereo, ori)
    assert got.tolist() == want.tolist() and st["n_matches"] == want_n
    return st


def _bow(k1, k2, nn_ratio, ori):
    want_n, want = kc.oracle_bow_kf(k1, k2, nn_ratio, ori)
    got, st = kr.search_by_bow_kf(k1, k2, nn_ratio, ori)
    assert got.tolist() == want.tolist() and st["n_matches"] == want_n
    return st


@pytest.mark.parametrize("name", sorted(kc.triangulation_hand_cases()))
def test_triangulation_hand_cases(name):
    k1, k2, geo, only_stereo, ori, want, want_n = kc.triangulation_hand_cases()[name]
    n, m = kc.oracle_triangulation(k1, k2, geo, *kc.HAND_LEVELS, only_stereo, ori)
    assert m.tolist() == want and n == want_n
    st = _tri(k1, k2, geo, kc.HAND_LEVELS, only_stereo, ori)
    expect = {"last_of_equal_wins": ("n_ties", 1), "both_taken": ("n_researched", 1), "both_taken_nothing_left": ("n_researched", 1),
              "best_taken_second_free": ("n_researched", 0), "best_taken_no_second": ("n_researched", 0), "line_outside": ("line_rejected", 1),
              "den_zero": ("line_rejected", 1), "inside_epipole_radius": ("epipole_rejected", 1), "at_epipole_radius": ("epipole_rejected", 0)}
    if name in expect:
        assert st[expect[name][0]] == expect[name][1]


@pytest.mark.parametrize("name", sorted(kc.bow_kf_hand_cases()))
def test_bow_kf_hand_cases(name):
    k1, k2, nn_ratio, ori, want, want_n = kc.bow_kf_hand_cases()[name]
    n, m = kc.oracle_bow_kf(k1, k2, nn_ratio, ori)
    assert m.tolist() == want and n == want_n
    st = _bow(k1, k2, nn_ratio, ori)
    if name == "first_of_equal_wins":
        assert st["n_ties"] == 1
    if name == "three_compete":
        assert st["n_researched"] == 2


@pytest.mark.parametrize("seed", [5, 6])
def test_random_pairs(seed):
    k1, k2, geo, lv = kc.random_pair(seed)
    ep = line = ties = 0
    for only_stereo in (0, 1):
        for a, b in ((k1, k2), (k2, k1)):
            st = _tri(a, b, geo, lv, only_stereo, 1)
            ep, line, ties = ep + st["epipole_rejected"], line + st["line_rejected"], ties + st["n_ties"]
    assert ep > 0 and line > 0  # both tests reject candidates that passed the distance test
    assert ties > 0             # an accepted match is the last of several candidates of one distance
    k1, k2, _, _ = kc.random_pair(seed, point_share=0.8)
    for ori in (0, 1):
        _bow(k1, k2, 0.75, ori)
        _bow(k2, k1, 0.75, ori)


@pytest.mark.parametrize("nodes", sorted(bc.NODE_LEVELS))
@pytest.mark.parametrize("size", sorted(bc.SIZES))
def test_synth_frames(ob, synth, size, nodes):
    """every (pair, only_stereo, orientation) the GPU tests run; on the large frames the inputs must exercise what the device form adds"""
    sides = kc.synth_sides(ob, synth, size, nodes, 0.3)
    geos, lv = kc.synth_geometry(size)
    res = {}
    for only_stereo in (0, 1):
        for ori in (0, 1):
            if size == "large" and (only_stereo, ori) != (0, 1):
                continue
            res[only_stereo, ori] = [_tri(sides[a], sides[b], geos[g], lv, only_stereo, ori) for (a, b), g in zip(kc.PAIRS, kc.PAIR_GEOMETRY)]
    sides_b = kc.synth_sides(ob, synth, size, nodes, 0.8)
    res_b = [_bow(sides_b[a], sides_b[b], 0.75, 1) for a, b in kc.PAIRS]
    if size == "small":
        for a, b in kc.PAIRS:
            _bow(sides_b[a], sides_b[b], 0.75, 0)
    if size == "large":
        tri = res[0, 1]
        print([{k: s[k] for k in s} for s in tri], [{k: s[k] for k in s} for s in res_b])
        assert all(s["n_matches"] >= 30 for s in tri) and all(s["n_matches"] >= 30 for s in res_b)
        assert any(s["n_researched"] > 0 for s in tri) and any(s["n_researched"] > 0 for s in res_b)
        assert any(s["line_rejected"] > 0 for s in tri)


def test_exports_and_mirror(pkg):
    L = pkg.lib()
    for name in ("amos_match_bow_kf_batch_device", "amos_match_triangulation_batch_device", "amos_match_bow_kf", "amos_match_triangulation"):
        assert name in pkg.EXPORTS and hasattr(L, name), name
    for name in ("bow_kf_batch_device", "bow_kf", "triangulation_batch_device", "triangulation"):
        assert callable(getattr(pkg.OrbMatcher, name))
    assert C.sizeof(pkg.KfPairSearch) == 13 * 8 + 8 and pkg.KF_GEOMETRY_DTYPE.itemsize == 44
    # NULL handles and arguments are AMOS_ERR_INVALID
    assert L.amos_match_bow_kf_batch_device(None, None, 0.75, 1) == -1
    assert L.amos_match_triangulation_batch_device(None, None, None, None, None, 8, 0, 1) == -1
    assert L.amos_match_bow_kf(None, None, None, 0.75, 1, None, None) == -1
    assert L.amos_match_triangulation(None, None, None, 1, None, None, None, 8, 0, 1, None, None) == -1


def test_host_forms_reject_broken_views_before_the_device(pkg):
    """the checks come before any device call: a handle that was never created (an address that is not one) is never dereferenced"""
    L = pkg.lib()
    k1, k2 = kc.bow_kf_hand_cases()["three_compete"][:2]
    good = kc.with_csr(k1)
    other, keep_o = pkg.OrbMatcher._bow_view(*[kc.with_csr(k2)[k] for k in ("keys", "desc", "node_ids", "node_off", "node_idx")])
    fake = C.c_void_p(0x10)  # read only after the checks have passed
    stats, m12 = np.zeros(2, pkg.BOW_SEARCH_STATS_DTYPE), np.zeros(8, np.int32)
    geo, (sf, sg) = np.zeros(2, pkg.KF_GEOMETRY_DTYPE), kc.HAND_LEVELS
    for bad in (dict(good, node_idx=np.array([0, 1, 3], np.int32)), dict(good, node_off=np.array([0, 4], np.int32)),
                dict(good, node_ids=np.array([5, 5], np.uint32), node_off=np.array([0, 1, 3], np.int32))):
        v, keep = pkg.OrbMatcher._bow_view(*[bad[k] for k in ("keys", "desc", "node_ids", "node_off", "node_idx")])
        assert L.amos_match_bow_kf(fake, C.byref(v), C.byref(other), 0.75, 1, pkg._p(m12), pkg._p(stats)) == -1
        assert L.amos_match_bow_kf(fake, C.byref(other), C.byref(v), 0.75, 1, pkg._p(m12), pkg._p(stats)) == -1
        assert L.amos_last_error().decode().startswith("amos_match_bow_kf")
        for first, rest in ((v, [other, other]), (other, [other, v])):
            ptrs = (C.c_void_p * 2)(*[C.addressof(r) for r in rest])
            assert L.amos_match_triangulation(fake, C.byref(first), ptrs, 2, pkg._p(geo), pkg._p(sf), pkg._p(sg), 8, 0, 1, pkg._p(m12), pkg._p(stats)) == -1
            assert L.amos_last_error().decode().startswith("amos_match_triangulation")
    ptrs = (C.c_void_p * 2)(C.addressof(other), C.addressof(other))
    for n2, nl in ((0, 8), (2, 0), (2, 17)):
        assert L.amos_match_triangulation(fake, C.byref(other), ptrs, n2, pkg._p(geo), pkg._p(sf), pkg._p(sg), nl, 0, 1, pkg._p(m12), pkg._p(stats)) == -1
