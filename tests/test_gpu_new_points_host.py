"""amos_match_new_points (the host form) and ORB_SLAM2::CreateNewMapPointCandidates (the C++ drop-in, on stand-in KeyFrame objects) on the
GPU against the restatement fed with the CPU oracle's matches: geometry and baseline gate per neighbour from the poses, the search, the
triangulation and the claim rule in one call; a gated neighbour among the others; the -1 refusal."""
import numpy as np
import pytest

import host_new_points_binding as hnb
import kf_search_cases as kc
import new_points_cases as nc
import new_points_restatement as nr

pytestmark = pytest.mark.gpu


def neighbours(kind="forward", seed=5):
    """keyframe 1 and three neighbours: the random case's two, and between them one that stands closer than its stereo baseline"""
    case = nc.random_case(seed, kind)
    k1, k2, k3 = case["sides"]
    cam1, cam2, cam3 = case["cams"]
    gated = cam2.copy()
    gated["tcw"] = gated["tcw"] * np.float32(0.1)
    gated["Ow"] = gated["Ow"] * np.float32(0.1)
    assert not nr.pair_geometry(cam1, gated)[1] and nr.pair_geometry(cam1, cam2)[1]
    return k1, [k2, k3, k2], cam1, [cam2, gated, cam3], case["levels"]


def same(got, want):
    return len(got) == len(want) and all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("kind", nc.RANDOM_KINDS)
def test_host_form(gpu_lib, kind):
    k1, k2s, cam1, cams2, lv = neighbours(kind)
    mt = gpu_lib.OrbMatcher()
    for ori in (0, 1):  # (the handle's staging is used twice)
        got, stats = mt.new_points(kc.with_csr(k1), [kc.with_csr(k) for k in k2s], cam1, np.stack(cams2), lv[0], lv[1], check_orientation=ori)
        want, want_stats, kept = nc.host_expected(k1, k2s, cam1, cams2, lv, 0, ori)
        print("n_new", stats["n_new"].tolist(), "verdicts", stats["n_verdict"].tolist())
        assert kept == [0, 2] and stats[1].tobytes() == bytes(64) and len(got[1]) == 0
        assert stats.tobytes() == want_stats.tobytes() and same(got, want)
        assert stats["n_new"][0] > 0 and stats["n_verdict"][2, nr.CLAIMED] > 0
    # one neighbour, and only gated ones
    got, stats = mt.new_points(kc.with_csr(k1), [kc.with_csr(k2s[0])], cam1, cams2[0], lv[0], lv[1])
    want, want_stats, _ = nc.host_expected(k1, k2s[:1], cam1, cams2[:1], lv)
    assert stats.tobytes() == want_stats.tobytes() and same(got, want)
    got, stats = mt.new_points(kc.with_csr(k1), [kc.with_csr(k2s[1])] * 2, cam1, np.stack([cams2[1]] * 2), lv[0], lv[1])
    assert stats.tobytes() == bytes(128) and all(len(g) == 0 for g in got)
    mt.close()


def test_host_form_without_raw_keys_and_without_stereo(gpu_lib):
    k1, k2s, cam1, cams2, lv = neighbours()
    mt = gpu_lib.OrbMatcher()
    for strip in (dict(keys_raw=None), dict(u_right=None, depth=None)):
        a1, a2s = dict(k1, **strip), [dict(k, **strip) for k in k2s]
        got, stats = mt.new_points(kc.with_csr(a1), [kc.with_csr(k) for k in a2s], cam1, np.stack(cams2), lv[0], lv[1])
        want, want_stats, _ = nc.host_expected(a1, a2s, cam1, cams2, lv)
        assert stats.tobytes() == want_stats.tobytes() and same(got, want)
    # a monocular view among stereo ones
    a2s = [k2s[0], k2s[1], dict(k2s[2], u_right=None, depth=None)]
    got, stats = mt.new_points(kc.with_csr(k1), [kc.with_csr(k) for k in a2s], cam1, np.stack(cams2), lv[0], lv[1])
    want, want_stats, _ = nc.host_expected(k1, a2s, cam1, cams2, lv)
    assert stats.tobytes() == want_stats.tobytes() and same(got, want)
    mt.close()


def test_host_form_on_the_synth_keyframes(gpu_lib, ob, synth):
    """one keyframe 1 against three neighbours of other sizes"""
    case = nc.synth_case(ob, synth)
    sides, cams, lv = case["sides"], case["cams"], case["levels"]
    mt = gpu_lib.OrbMatcher()
    got, stats = mt.new_points(kc.with_csr(sides[1]), [kc.with_csr(sides[k]) for k in (0, 2, 3)], cams[1], np.stack([cams[k] for k in (0, 2, 3)]), lv[0],
                               lv[1], check_orientation=True)
    mt.close()
    want, want_stats, kept = nc.host_expected(sides[1], [sides[k] for k in (0, 2, 3)], cams[1], [cams[k] for k in (0, 2, 3)], lv, 0, 1)
    print("n_new", stats["n_new"].tolist(), "verdicts", stats["n_verdict"].tolist())
    assert kept == [0, 1, 2] and stats.tobytes() == want_stats.tobytes() and same(got, want) and stats["n_new"].sum() > 0


@pytest.mark.parametrize("kind", nc.RANDOM_KINDS)
def test_dropin_on_standin_keyframes(gpu_lib, kind):
    """CreateNewMapPointCandidates == the restatement; and == what the mapping thread ran before (the drop-in search, then the
    host-compiled core over neighbours and matches)"""
    k1, k2s, cam1, cams2, lv = neighbours(kind)
    case = {"sides": [k1] + k2s, "cams": [cam1] + cams2, "levels": lv}
    want, want_stats, kept = nc.host_expected(k1, k2s, cam1, cams2, lv, 0, 0)
    ret, got, stats, _ = hnb.dropin("dropin", case)
    assert ret == int(want_stats["n_new"].sum()) > 0 and same(got, want) and stats.tobytes() == want_stats.tobytes()
    ret_parent, got_parent, _, _ = hnb.dropin("parent", case)
    assert ret_parent == ret and same(got_parent, want)


def test_dropin_refusal(gpu_lib):
    """a stereo keyframe without depths: the library refuses, the drop-in returns -1 and its text"""
    k1, k2s, cam1, cams2, lv = neighbours()
    case = {"sides": [k1, dict(k2s[0], depth=None)], "cams": [cam1, cams2[0]], "levels": lv}
    with pytest.raises(RuntimeError, match="amos_match_new_points: invalid argument"):
        hnb.dropin("dropin", case)
    mt = gpu_lib.OrbMatcher()
    with pytest.raises(gpu_lib.AmosError, match="rc=-1"):
        mt.new_points(kc.with_csr(k1), [kc.with_csr(dict(k2s[0], depth=None))], cam1, cams2[0], lv[0], lv[1])
    good = kc.with_csr(k2s[0])
    with pytest.raises(gpu_lib.AmosError, match="rc=-1"):
        mt.new_points(kc.with_csr(k1), [good, dict(good, node_idx=np.full(len(good["node_idx"]), len(k2s[0]["desc"]), np.int32))], cam1,
                      np.stack(cams2[:2]), lv[0], lv[1])
    mt.close()
