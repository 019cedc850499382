"""amos_match_triangulation_batch_device / amos_match_bow_kf_batch_device and their host forms on the GPU against the CPU oracle
(orc_search_for_triangulation, orc_search_by_bow_kf): d_match12 with its padding and the return value, bit for bit; n_queries and
n_researched against the plain-Python replay (tests/kf_search_restatement.py), which is itself held to the oracle here and in
test_kf_search_cpu.py."""
import numpy as np
import pytest

import bow_search_cases as bc
import kf_search_cases as kc
import kf_search_restatement as kr

pytestmark = pytest.mark.gpu

STAT_FIELDS = kc.STAT_FIELDS


def _up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()


def run_device(pkg, which, sides, pairs, pad=5, with_has_point=True, with_u_right=True, mt=None, **kw):
    """which: "tri" (kw: geos [pairs], levels, only_stereo, ori) or "bow" (kw: nn_ratio, ori) -> (match12 [pairs][cap], stats)"""
    import torch
    cap = max(max(len(s["desc"]) for s in sides), 1) + pad
    d = {k: _up(v) for k, v in kc.pack(sides, cap, 0 if which == "tri" else 1).items()}
    d_1, d_2 = _up(np.array([p[0] for p in pairs], np.int32)), _up(np.array([p[1] for p in pairs], np.int32))
    d_match = torch.full((len(pairs), cap), 12345, dtype=torch.int32, device="cuda")  # the call itself resets it
    d_stats = torch.full((len(pairs), 4), -9, dtype=torch.int32, device="cuda")
    common = (d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d["n_nodes"].data_ptr(), d["node_ids"].data_ptr(),
              d["node_off"].data_ptr(), d["node_idx"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(), len(pairs), cap)
    hp = d["has_point"].data_ptr() if with_has_point else None
    own = mt is None
    mt = mt or pkg.OrbMatcher()
    if which == "tri":
        sf, sg = kw["levels"]
        d_geo, d_sf, d_sg = _up(np.stack(kw["geos"])), _up(sf), _up(sg)
        torch.cuda.synchronize()
        mt.triangulation_batch_device(*common, d_geo.data_ptr(), d_sf.data_ptr(), d_sg.data_ptr(), kw.get("n_levels", len(sf)), d_match.data_ptr(),
                                      d_stats.data_ptr(), only_stereo=kw["only_stereo"], check_orientation=kw["ori"], d_has_point=hp,
                                      d_u_right=d["u_right"].data_ptr() if with_u_right else None)
    else:
        torch.cuda.synchronize()
        mt.bow_kf_batch_device(*common, d_match.data_ptr(), d_stats.data_ptr(), nn_ratio=kw["nn_ratio"], check_orientation=kw["ori"], d_has_point=hp)
    mt.sync()
    match = d_match.cpu().numpy()
    stats = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.BOW_SEARCH_STATS_DTYPE)
    if own:
        mt.close()
    return match, stats


def _without(s, has_point, u_right):
    s = dict(s)
    if not has_point:
        s["has_point"] = None
    if not u_right:
        s["u_right"] = None
    return s


def check_tri(pkg, sides, pairs, geos, lv, only_stereo, ori, with_has_point=True, with_u_right=True, mt=None):
    match, stats = run_device(pkg, "tri", sides, pairs, geos=geos, levels=lv, only_stereo=only_stereo, ori=ori, with_has_point=with_has_point,
                              with_u_right=with_u_right, mt=mt)
    out = []
    for p, ((i1, i2), g) in enumerate(zip(pairs, geos)):
        k1, k2 = _without(sides[i1], with_has_point, with_u_right), _without(sides[i2], with_has_point, with_u_right)
        want_n, want = kc.oracle_triangulation(k1, k2, g, lv[0], lv[1], only_stereo, ori)
        replay, rs = kr.search_for_triangulation(k1, k2, g["f12"], g["ex"], g["ey"], lv[0], lv[1], only_stereo, ori)
        print(f"pair {p} ({i1} -> {i2}): oracle {want_n} matches, device " + ", ".join(f"{k} {stats[k][p]} / {rs[k]}" for k in STAT_FIELDS)
              + f", status {stats['status'][p]}")
        assert replay.tolist() == want.tolist() and rs["n_matches"] == want_n  # the replay is the oracle's loop
        n = len(k1["desc"])
        assert np.array_equal(match[p, :n], want), p
        assert (match[p, n:] == -1).all(), p
        assert tuple(int(stats[k][p]) for k in STAT_FIELDS) == tuple(rs[k] for k in STAT_FIELDS), p
        assert stats["status"][p] == 0
        out.append(rs)
    return out


def check_bow(pkg, sides, pairs, nn_ratio, ori, with_has_point=True, mt=None):
    match, stats = run_device(pkg, "bow", sides, pairs, nn_ratio=nn_ratio, ori=ori, with_has_point=with_has_point, mt=mt)
    out = []
    for p, (i1, i2) in enumerate(pairs):
        k1, k2 = _without(sides[i1], with_has_point, True), _without(sides[i2], with_has_point, True)
        want_n, want = kc.oracle_bow_kf(k1, k2, nn_ratio, ori)
        replay, rs = kr.search_by_bow_kf(k1, k2, nn_ratio, ori)
        print(f"pair {p} ({i1} -> {i2}): oracle {want_n} matches, device " + ", ".join(f"{k} {stats[k][p]} / {rs[k]}" for k in STAT_FIELDS)
              + f", status {stats['status'][p]}")
        assert replay.tolist() == want.tolist() and rs["n_matches"] == want_n
        n = len(k1["desc"])
        assert np.array_equal(match[p, :n], want), p
        assert (match[p, n:] == -1).all(), p
        assert tuple(int(stats[k][p]) for k in STAT_FIELDS) == tuple(rs[k] for k in STAT_FIELDS), p
        assert stats["status"][p] == 0
        out.append(rs)
    return out


# ---------------------------------------------------------------------------------------------------------------- triangulation

@pytest.mark.parametrize("ori", [0, 1])
@pytest.mark.parametrize("only_stereo", [0, 1])
@pytest.mark.parametrize("nodes", sorted(bc.NODE_LEVELS))
def test_triangulation_synth_small(gpu_lib, ob, synth, nodes, only_stereo, ori):
    """four pairs in one call, three of them against one keyframe 1, each with its own geometry"""
    sides = kc.synth_sides(ob, synth, "small", nodes, 0.3)
    geos, lv = kc.synth_geometry("small")
    check_tri(gpu_lib, sides, kc.PAIRS, [geos[g] for g in kc.PAIR_GEOMETRY], lv, only_stereo, ori)


@pytest.mark.parametrize("nodes", sorted(bc.NODE_LEVELS))
def test_triangulation_synth_large(gpu_lib, ob, synth, nodes):
    sides = kc.synth_sides(ob, synth, "large", nodes, 0.3)
    geos, lv = kc.synth_geometry("large")
    res = check_tri(gpu_lib, sides, kc.PAIRS, [geos[g] for g in kc.PAIR_GEOMETRY], lv, 0, 1)
    assert all(rs["n_matches"] >= 30 for rs in res)  # what the inputs must exercise
    assert any(rs["n_researched"] > 0 for rs in res) and any(rs["line_rejected"] > 0 for rs in res)


@pytest.mark.parametrize("only_stereo", [0, 1])
@pytest.mark.parametrize("seed", [5, 6])
def test_triangulation_random_pairs(gpu_lib, seed, only_stereo):
    """70 x 80 features in 4 nodes, an epipole inside the image; the capacity fills neither a wave nor a work-group; one handle, two calls"""
    k1, k2, geo, lv = kc.random_pair(seed)
    mt = gpu_lib.OrbMatcher()
    res = check_tri(gpu_lib, [k1, k2], [(0, 1), (1, 0)], [geo, geo], lv, only_stereo, 1, mt=mt)
    res += check_tri(gpu_lib, [k1, k2], [(1, 0)], [geo], lv, only_stereo, 0, mt=mt)
    mt.close()
    if not only_stereo:
        assert sum(rs["epipole_rejected"] for rs in res) > 0 and sum(rs["line_rejected"] for rs in res) > 0
        assert sum(rs["n_ties"] for rs in res) > 0


def test_triangulation_without_optional_arrays(gpu_lib):
    """d_has_point NULL: no feature has a map point; d_u_right NULL: every feature is mono"""
    k1, k2, geo, lv = kc.random_pair(6)
    check_tri(gpu_lib, [k1, k2], [(0, 1)], [geo], lv, 0, 1, with_has_point=False, with_u_right=False)
    res = check_tri(gpu_lib, [k1, k2], [(0, 1)], [geo], lv, 1, 1, with_has_point=False, with_u_right=False)
    assert res[0]["n_queries"] == 0


@pytest.mark.parametrize("name", sorted(kc.triangulation_hand_cases()))
def test_triangulation_hand_cases(gpu_lib, name):
    k1, k2, geo, only_stereo, ori, want, want_n = kc.triangulation_hand_cases()[name]
    lv = kc.HAND_LEVELS
    oracle_n, oracle = kc.oracle_triangulation(k1, k2, geo, lv[0], lv[1], only_stereo, ori)
    assert oracle.tolist() == want and oracle_n == want_n  # the expectation written in the case is the oracle's
    hp = k1.get("has_point") is not None or k2.get("has_point") is not None
    ur = k1.get("u_right") is not None or k2.get("u_right") is not None
    check_tri(gpu_lib, [k1, k2], [(0, 1)], [geo], lv, only_stereo, ori, with_has_point=hp, with_u_right=ur)
    # the host form, from the views
    mt = gpu_lib.OrbMatcher()
    got, stats = mt.triangulation(kc.with_csr(k1), [kc.with_csr(k2)], [geo], lv[0], lv[1], only_stereo, ori)
    mt.close()
    _, rs = kr.search_for_triangulation(k1, k2, geo["f12"], geo["ex"], geo["ey"], lv[0], lv[1], only_stereo, ori)
    assert got[0].tolist() == want and tuple(int(stats[k][0]) for k in STAT_FIELDS) == tuple(rs[k] for k in STAT_FIELDS) and stats["status"][0] == 0


def test_triangulation_host_form_one_against_three(gpu_lib, ob, synth):
    """the LocalMapping shape: one keyframe 1 against three neighbours in ONE call; the handle's staging is used twice"""
    sides = kc.synth_sides(ob, synth, "small", "10", 0.3)
    geos, lv = kc.synth_geometry("small")
    pairs, kinds = kc.PAIRS[:3], kc.PAIR_GEOMETRY[:3]
    assert all(a == pairs[0][0] for a, _ in pairs)
    mt = gpu_lib.OrbMatcher()
    for only_stereo in (0, 1):
        got, stats = mt.triangulation(kc.with_csr(sides[pairs[0][0]]), [kc.with_csr(sides[b]) for _, b in pairs], [geos[g] for g in kinds],
                                      lv[0], lv[1], only_stereo, 1)
        for p, ((a, b), g) in enumerate(zip(pairs, kinds)):
            want_n, want = kc.oracle_triangulation(sides[a], sides[b], geos[g], lv[0], lv[1], only_stereo, 1)
            _, rs = kr.search_for_triangulation(sides[a], sides[b], geos[g]["f12"], geos[g]["ex"], geos[g]["ey"], lv[0], lv[1], only_stereo, 1)
            assert got[p].tolist() == want.tolist()
            assert tuple(int(stats[k][p]) for k in STAT_FIELDS) == (rs["n_queries"], want_n, rs["n_researched"]) and stats["status"][p] == 0
    # views of different sizes and a monocular view among stereo ones
    small, _, geo, lv2 = kc.random_pair(5)
    k2s = [dict(sides[0], u_right=None), small, sides[2]]
    got, stats = mt.triangulation(kc.with_csr(sides[1]), [kc.with_csr(k) for k in k2s], [geos["x"], geo, geos["y"]], lv2[0], lv2[1], 0, 1)
    for p, (k2, g) in enumerate(zip(k2s, [geos["x"], geo, geos["y"]])):
        want_n, want = kc.oracle_triangulation(sides[1], k2, g, lv2[0], lv2[1], 0, 1)
        assert got[p].tolist() == want.tolist() and stats["n_matches"][p] == want_n
    mt.close()


def test_triangulation_out_of_range_octave_and_index(gpu_lib):
    """the batch form cannot check device arrays: a keyframe-2 keypoint with an octave outside the levels is no candidate (status bit 1), a
    keyframe-1 index outside the keyframe is skipped (status bit 0), a keyframe-2 index outside is no candidate; everything else is the
    oracle's result on the inputs without them"""
    k1, k2, geo, lv = kc.random_pair(5)
    n1, n2 = len(k1["desc"]), len(k2["desc"])
    clean_n, clean = kc.oracle_triangulation(k1, k2, geo, lv[0], lv[1], 0, 1)
    node1, node2 = sorted(k1["fv"])[0], sorted(set(k1["fv"]) & set(k2["fv"]))[0]
    k1_bad = dict(k1, fv={k: (v + [n1, 1 << 30, -1] if k == node1 else v) for k, v in k1["fv"].items()})
    k2_bad = dict(k2, fv={k: ([n2, -5] + v if k == node2 else v) for k, v in k2["fv"].items()})
    match, stats = run_device(gpu_lib, "tri", [k1_bad, k2_bad], [(0, 1)], pad=7, geos=[geo], levels=lv, only_stereo=0, ori=1)
    assert np.array_equal(match[0, :n1], clean) and (match[0, n1:] == -1).all()
    assert stats["n_matches"][0] == clean_n and stats["status"][0] == gpu_lib.KF_STATUS_BAD_INDEX
    # octaves: the matched keyframe-2 features of the clean run get octaves 8 and -1; without them as candidates the result is the oracle's
    # with those features marked as having a map point (no candidate either)
    victims = clean[clean >= 0][:4]
    keys = k2["keys"].copy()
    keys["octave"][victims] = [8, -1, 8, 1 << 20][:len(victims)]
    hp = k2["has_point"].copy()
    hp[victims] = 1
    want_n, want = kc.oracle_triangulation(k1, dict(k2, has_point=hp), geo, lv[0], lv[1], 0, 1)
    match, stats = run_device(gpu_lib, "tri", [k1, dict(k2, keys=keys)], [(0, 1)], geos=[geo], levels=lv, only_stereo=0, ori=1)
    assert len(victims) == 4 and np.array_equal(match[0, :n1], want) and stats["n_matches"][0] == want_n
    assert stats["status"][0] == gpu_lib.KF_STATUS_BAD_OCTAVE


def test_transform_then_triangulation_on_the_device(gpu_lib, ob, synth):
    """ComputeBoW and SearchForTriangulation chained without a host copy between them == restatement -> oracle"""
    import torch
    sides = kc.synth_sides(ob, synth, "small", "100", 0.3)
    geos, lv = kc.synth_geometry("small")
    voc, lu = bc.vocabulary(), bc.NODE_LEVELS["100"]
    cap = max(len(s["desc"]) for s in sides) + 4
    a = kc.pack(sides, cap)
    ns, pairs = len(sides), kc.PAIRS
    d_kps, d_desc, d_counts, d_hp, d_ur = _up(a["kps"]), _up(a["desc"]), _up(a["counts"]), _up(a["has_point"]), _up(a["u_right"])
    i32 = dict(dtype=torch.int32, device="cuda")
    d_fw, d_fn, d_ids, d_idx, d_words = (torch.zeros((ns, cap), **i32) for _ in range(5))
    d_off, d_nn, d_nw = torch.zeros((ns, cap + 1), **i32), torch.zeros(ns, **i32), torch.zeros(ns, **i32)
    d_wts, d_bstats = torch.zeros((ns, cap), dtype=torch.float64, device="cuda"), torch.zeros((ns, 4), **i32)
    d_1, d_2 = _up(np.array([p[0] for p in pairs], np.int32)), _up(np.array([p[1] for p in pairs], np.int32))
    d_geo, d_sf, d_sg = _up(np.stack([geos[g] for g in kc.PAIR_GEOMETRY])), _up(lv[0]), _up(lv[1])
    d_match, d_stats = torch.full((len(pairs), cap), 777, **i32), torch.zeros((len(pairs), 4), **i32)
    torch.cuda.synchronize()
    mt = gpu_lib.OrbMatcher()
    bow = gpu_lib.BowVocabulary(voc.k, voc.L, *voc.arrays(), stream=mt.stream)  # one stream orders the two calls
    bow.transform_batch_device(d_desc.data_ptr(), d_counts.data_ptr(), ns, cap, lu, d_fw.data_ptr(), d_fn.data_ptr(), d_nn.data_ptr(),
                               d_ids.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), d_nw.data_ptr(), d_words.data_ptr(), d_wts.data_ptr(),
                               d_bstats.data_ptr())
    mt.triangulation_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_nn.data_ptr(), d_ids.data_ptr(), d_off.data_ptr(),
                                  d_idx.data_ptr(), d_1.data_ptr(), d_2.data_ptr(), len(pairs), cap, d_geo.data_ptr(), d_sf.data_ptr(),
                                  d_sg.data_ptr(), len(lv[0]), d_match.data_ptr(), d_stats.data_ptr(), only_stereo=False, check_orientation=True,
                                  d_has_point=d_hp.data_ptr(), d_u_right=d_ur.data_ptr())
    mt.sync()
    match = d_match.cpu().numpy()
    stats = np.frombuffer(d_stats.cpu().numpy().tobytes(), gpu_lib.BOW_SEARCH_STATS_DTYPE)
    bow.close()
    mt.close()
    for p, ((i1, i2), g) in enumerate(zip(pairs, kc.PAIR_GEOMETRY)):
        want_n, want = kc.oracle_triangulation(sides[i1], sides[i2], geos[g], lv[0], lv[1], 0, 1)
        assert np.array_equal(match[p, :len(want)], want) and (match[p, len(want):] == -1).all() and stats["n_matches"][p] == want_n


# ---------------------------------------------------------------------------------------------------------------- SearchByBoW(KF, KF)

@pytest.mark.parametrize("ori", [0, 1])
@pytest.mark.parametrize("nodes", sorted(bc.NODE_LEVELS))
def test_bow_kf_synth_small(gpu_lib, ob, synth, nodes, ori):
    sides = kc.synth_sides(ob, synth, "small", nodes, 0.8)
    check_bow(gpu_lib, sides, kc.PAIRS, 0.75, ori)


@pytest.mark.parametrize("nodes", sorted(bc.NODE_LEVELS))
def test_bow_kf_synth_large(gpu_lib, ob, synth, nodes):
    sides = kc.synth_sides(ob, synth, "large", nodes, 0.8)
    res = check_bow(gpu_lib, sides, kc.PAIRS, 0.75, 1)
    assert all(rs["n_matches"] >= 30 for rs in res) and any(rs["n_researched"] > 0 for rs in res)


@pytest.mark.parametrize("seed", [5, 6])
def test_bow_kf_random_pairs(gpu_lib, seed):
    k1, k2, _, _ = kc.random_pair(seed, point_share=0.8)
    mt = gpu_lib.OrbMatcher()
    check_bow(gpu_lib, [k1, k2], [(0, 1), (1, 0)], 0.75, 1, mt=mt)
    check_bow(gpu_lib, [k1, k2], [(0, 1)], 0.6, 0, with_has_point=False, mt=mt)  # the handle is used twice; NULL: every feature has a point
    mt.close()


@pytest.mark.parametrize("name", sorted(kc.bow_kf_hand_cases()))
def test_bow_kf_hand_cases(gpu_lib, name):
    k1, k2, nn_ratio, ori, want, want_n = kc.bow_kf_hand_cases()[name]
    oracle_n, oracle = kc.oracle_bow_kf(k1, k2, nn_ratio, ori)
    assert oracle.tolist() == want and oracle_n == want_n
    hp = k1.get("has_point") is not None or k2.get("has_point") is not None
    check_bow(gpu_lib, [k1, k2], [(0, 1)], nn_ratio, ori, with_has_point=hp)
    mt = gpu_lib.OrbMatcher()
    got, stats = mt.bow_kf(kc.with_csr(k1), kc.with_csr(k2), nn_ratio, ori)
    mt.close()
    _, rs = kr.search_by_bow_kf(k1, k2, nn_ratio, ori)
    assert got.tolist() == want and tuple(int(stats[k]) for k in STAT_FIELDS) == tuple(rs[k] for k in STAT_FIELDS) and stats["status"] == 0


def test_bow_kf_host_form_on_synth_frames(gpu_lib, ob, synth):
    sides = kc.synth_sides(ob, synth, "small", "10", 0.8)
    mt = gpu_lib.OrbMatcher()
    for k2 in (sides[0], dict(sides[2], has_point=None)):  # the handle's staging is used twice; one view without has_point among two
        got, stats = mt.bow_kf(kc.with_csr(sides[1]), kc.with_csr(k2), 0.75, 1)
        want_n, want = kc.oracle_bow_kf(sides[1], k2, 0.75, 1)
        _, rs = kr.search_by_bow_kf(sides[1], k2, 0.75, 1)
        assert got.tolist() == want.tolist() and tuple(int(stats[k]) for k in STAT_FIELDS) == (rs["n_queries"], want_n, rs["n_researched"])
    mt.close()


def test_bow_kf_out_of_range_feature_index(gpu_lib):
    k1, k2, _, _ = kc.random_pair(5, point_share=0.8)
    n1, n2 = len(k1["desc"]), len(k2["desc"])
    clean_n, clean = kc.oracle_bow_kf(k1, k2, 0.75, 1)
    node1, node2 = sorted(k1["fv"])[0], sorted(set(k1["fv"]) & set(k2["fv"]))[0]
    k1_bad = dict(k1, fv={k: (v + [n1, 1 << 30, -1] if k == node1 else v) for k, v in k1["fv"].items()})
    k2_bad = dict(k2, fv={k: ([n2, -5] + v if k == node2 else v) for k, v in k2["fv"].items()})
    match, stats = run_device(gpu_lib, "bow", [k1_bad, k2_bad], [(0, 1)], pad=7, nn_ratio=0.75, ori=1)
    assert np.array_equal(match[0, :n1], clean) and (match[0, n1:] == -1).all()
    assert stats["n_matches"][0] == clean_n and stats["status"][0] == gpu_lib.KF_STATUS_BAD_INDEX


def test_host_forms_reject_a_broken_view(gpu_lib):
    k1, k2 = kc.bow_kf_hand_cases()["three_compete"][:2]
    mt = gpu_lib.OrbMatcher()
    good, sf, sg = kc.with_csr(k1), *kc.HAND_LEVELS
    for bad in (dict(good, node_idx=np.array([0, 1, 3], np.int32)), dict(good, node_off=np.array([0, 4], np.int32)),
                dict(good, node_ids=np.array([5, 5], np.uint32), node_off=np.array([0, 1, 3], np.int32))):
        with pytest.raises(gpu_lib.AmosError, match="rc=-1"):
            mt.bow_kf(bad, kc.with_csr(k2))
        with pytest.raises(gpu_lib.AmosError, match="rc=-1"):
            mt.triangulation(kc.with_csr(k2), [kc.with_csr(k2), bad], [kc.G_X, kc.G_X], sf, sg)
    mt.close()
