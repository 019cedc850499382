"""amos_match_bow_batch_device / amos_match_bow on the GPU against orc_search_by_bow (oracle/orb_oracle.c): d_match with its padding and the
return value; n_queries and n_researched against the plain-Python replay of the same loop (tests/bow_restatement.py), which is itself held
to the oracle's matches here and in test_bow_cpu.py."""
import numpy as np
import pytest

import bow_restatement as br
import bow_search_cases as bc

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("n_queries", "n_matches", "n_researched")


def pack(pkg, sides, cap):
    """the resident arrays of the frame slots: kps, desc, counts, n_nodes, node_ids, node_off, node_idx, has_point (1 where a side has none)"""
    ns = len(sides)
    a = dict(kps=np.zeros((ns, cap), pkg.KP_DTYPE), desc=np.full((ns, cap, 32), 0x3C, np.uint8), counts=np.zeros(ns, np.int32),
             n_nodes=np.zeros(ns, np.int32), node_ids=np.full((ns, cap), 0xABABABAB, np.uint32), node_off=np.full((ns, cap + 1), -77, np.int32),
             node_idx=np.full((ns, cap), -55, np.int32), has_point=np.ones((ns, cap), np.uint8))
    for s, sd in enumerate(sides):
        n = len(sd["desc"])
        ids, off, idx = bc.csr(sd["fv"])
        a["counts"][s], a["n_nodes"][s] = n, len(ids)
        a["kps"][s, :n], a["desc"][s, :n] = sd["keys"], sd["desc"]
        a["node_ids"][s, :len(ids)], a["node_off"][s, :len(off)], a["node_idx"][s, :len(idx)] = ids, off, idx
        if sd.get("has_point") is not None:
            a["has_point"][s, :n] = sd["has_point"]
    return a


def run_device(pkg, sides, pairs, nn_ratio, ori, with_has_point, pad=5):
    import torch
    cap = max(max(len(s["desc"]) for s in sides), 1) + pad
    a = pack(pkg, sides, cap)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    d = {k: up(v) for k, v in a.items()}
    d_kf, d_f = up(np.array([p[0] for p in pairs], np.int32)), up(np.array([p[1] for p in pairs], np.int32))
    d_match = torch.full((len(pairs), cap), 12345, dtype=torch.int32, device="cuda")  # the call itself resets it
    d_stats = torch.full((len(pairs), 4), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mt = pkg.OrbMatcher()
    mt.bow_batch_device(d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d["n_nodes"].data_ptr(), d["node_ids"].data_ptr(),
                        d["node_off"].data_ptr(), d["node_idx"].data_ptr(), d_kf.data_ptr(), d_f.data_ptr(), len(pairs), cap, d_match.data_ptr(),
                        d_stats.data_ptr(), nn_ratio=nn_ratio, check_orientation=ori, d_has_point=d["has_point"].data_ptr() if with_has_point else None)
    mt.sync()
    match = d_match.cpu().numpy()
    stats = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.BOW_SEARCH_STATS_DTYPE)
    mt.close()
    return match, stats


def check_pairs(pkg, ob, sides, pairs, nn_ratio, ori, with_has_point):
    match, stats = run_device(pkg, sides, pairs, nn_ratio, ori, with_has_point)
    out = []
    for p, (ikf, i_f) in enumerate(pairs):
        kf = dict(sides[ikf]) if with_has_point else dict(sides[ikf], has_point=None)
        f = sides[i_f]
        want_n, want = bc.oracle_search(ob, kf, f, nn_ratio, ori)
        replay, rs = br.search_by_bow(kf, f, nn_ratio, ori)
        print(f"pair {p} ({ikf} -> {i_f}): oracle {want_n} matches, device " + ", ".join(f"{k} {stats[k][p]} / {rs[k]}" for k in STAT_FIELDS)
              + f", status {stats['status'][p]}")
        assert replay.tolist() == want.tolist() and rs["n_matches"] == want_n  # the replay is the oracle's loop
        n = len(f["desc"])
        assert np.array_equal(match[p, :n], want), p
        assert (match[p, n:] == -1).all(), p
        assert tuple(int(stats[k][p]) for k in STAT_FIELDS) == tuple(rs[k] for k in STAT_FIELDS), p
        assert stats["status"][p] == 0
        out.append((want_n, rs))
    return out


@pytest.mark.parametrize("nn_ratio", [0.7, 0.75])
@pytest.mark.parametrize("ori", [0, 1])
@pytest.mark.parametrize("with_has_point", [False, True], ids=["all_points", "has_point_80"])
@pytest.mark.parametrize("nodes", sorted(bc.NODE_LEVELS))
@pytest.mark.parametrize("size", sorted(bc.SIZES))
def test_synth_frames(gpu_lib, ob, synth, size, nodes, with_has_point, ori, nn_ratio):
    """four pairs in one call, three of them keyframes against one frame"""
    sides = bc.synth_sides(ob, synth, size, nodes)
    res = check_pairs(gpu_lib, ob, sides, bc.PAIRS, nn_ratio, ori, with_has_point)
    if size == "large":  # what the inputs must exercise
        assert all(n >= 30 for n, _ in res)
        assert any(rs["n_researched"] > 0 for _, rs in res)


@pytest.mark.parametrize("name", sorted(bc.hand_cases()))
def test_hand_cases(gpu_lib, ob, name):
    kf, f, nn_ratio, ori, want, want_n = bc.hand_cases()[name]
    oracle_n, oracle = bc.oracle_search(ob, kf, f, nn_ratio, ori)
    assert oracle.tolist() == want and oracle_n == want_n  # the expectation written in the case is the oracle's
    check_pairs(gpu_lib, ob, [kf, f], [(0, 1)], nn_ratio, ori, kf.get("has_point") is not None)
    # the host form, from the views
    mt = gpu_lib.OrbMatcher()
    got, stats = mt.bow(bc.with_csr(kf), bc.with_csr(f), nn_ratio, ori)
    mt.close()
    _, rs = br.search_by_bow(kf, f, nn_ratio, ori)
    assert got.tolist() == want and tuple(int(stats[k]) for k in STAT_FIELDS) == tuple(rs[k] for k in STAT_FIELDS) and stats["status"] == 0


@pytest.mark.parametrize("with_has_point", [False, True])
def test_host_form_on_synth_frames(gpu_lib, ob, synth, with_has_point):
    sides = bc.synth_sides(ob, synth, "small", "10")
    kf = dict(sides[0]) if with_has_point else dict(sides[0], has_point=None)
    mt = gpu_lib.OrbMatcher()
    for f in (sides[1], sides[2]):  # the handle's staging is used twice
        got, stats = mt.bow(bc.with_csr(kf), bc.with_csr(f), 0.7, 1)
        want_n, want = bc.oracle_search(ob, kf, f, 0.7, 1)
        _, rs = br.search_by_bow(kf, f, 0.7, 1)
        assert got.tolist() == want.tolist() and tuple(int(stats[k]) for k in STAT_FIELDS) == (rs["n_queries"], want_n, rs["n_researched"])
    mt.close()


def test_host_form_rejects_a_broken_view(gpu_lib):
    kf, f = bc.hand_cases()["three_compete"][:2]
    mt = gpu_lib.OrbMatcher()
    good = bc.with_csr(kf)
    for bad in (dict(good, node_idx=np.array([0, 1, 3], np.int32)), dict(good, node_off=np.array([0, 4], np.int32)),
                dict(good, node_ids=np.array([5, 5], np.uint32), node_off=np.array([0, 1, 3], np.int32))):
        with pytest.raises(gpu_lib.AmosError, match="rc=-1"):
            mt.bow(bad, bc.with_csr(f))
    mt.close()


def test_out_of_range_feature_index_is_not_dereferenced(gpu_lib, ob):
    """the batch form cannot check device arrays: a keyframe index outside the keyframe is skipped and reported, a frame index outside the
    frame is no candidate; everything else is the oracle's result on the lists without them"""
    kf, f = bc.random_pair(5, 70, 80, 4)
    clean_n, clean = bc.oracle_search(ob, kf, f, 0.7, 1)
    node_kf, node_f = sorted(kf["fv"])[0], sorted(set(kf["fv"]) & set(f["fv"]))[0]
    kf_bad = dict(kf, fv={k: (v + [70, 1 << 30, -1] if k == node_kf else v) for k, v in kf["fv"].items()})
    f_bad = dict(f, fv={k: ([80, -5] + v if k == node_f else v) for k, v in f["fv"].items()})
    match, stats = run_device(gpu_lib, [kf_bad, f_bad], [(0, 1)], 0.7, 1, False, pad=7)
    assert np.array_equal(match[0, :80], clean) and (match[0, 80:] == -1).all()
    assert stats["n_matches"][0] == clean_n and stats["status"][0] == 1


def test_transform_then_search_on_the_device(gpu_lib, ob, synth):
    """ComputeBoW and SearchByBoW chained without a host copy between them == restatement -> oracle"""
    import torch
    sides = bc.synth_sides(ob, synth, "small", "100")
    voc, lu = bc.vocabulary(), bc.NODE_LEVELS["100"]
    cap = max(len(s["desc"]) for s in sides) + 4
    a = pack(gpu_lib, sides, cap)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    ns = len(sides)
    d_kps, d_desc, d_counts = up(a["kps"]), up(a["desc"]), up(a["counts"])
    i32 = dict(dtype=torch.int32, device="cuda")
    d_fw, d_fn, d_ids, d_idx, d_words = (torch.zeros((ns, cap), **i32) for _ in range(5))
    d_off, d_nn, d_nw = torch.zeros((ns, cap + 1), **i32), torch.zeros(ns, **i32), torch.zeros(ns, **i32)
    d_wts, d_bstats = torch.zeros((ns, cap), dtype=torch.float64, device="cuda"), torch.zeros((ns, 4), **i32)
    d_kf, d_f = up(np.array([p[0] for p in bc.PAIRS], np.int32)), up(np.array([p[1] for p in bc.PAIRS], np.int32))
    d_match, d_stats = torch.full((len(bc.PAIRS), cap), 777, **i32), torch.zeros((len(bc.PAIRS), 4), **i32)
    torch.cuda.synchronize()
    mt = gpu_lib.OrbMatcher()
    bow = gpu_lib.BowVocabulary(voc.k, voc.L, *voc.arrays(), stream=mt.stream)  # one stream orders the two calls
    bow.transform_batch_device(d_desc.data_ptr(), d_counts.data_ptr(), ns, cap, lu, d_fw.data_ptr(), d_fn.data_ptr(), d_nn.data_ptr(),
                               d_ids.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), d_nw.data_ptr(), d_words.data_ptr(), d_wts.data_ptr(),
                               d_bstats.data_ptr())
    mt.bow_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_nn.data_ptr(), d_ids.data_ptr(), d_off.data_ptr(),
                        d_idx.data_ptr(), d_kf.data_ptr(), d_f.data_ptr(), len(bc.PAIRS), cap, d_match.data_ptr(), d_stats.data_ptr(), nn_ratio=0.7,
                        check_orientation=1)
    mt.sync()
    match = d_match.cpu().numpy()
    stats = np.frombuffer(d_stats.cpu().numpy().tobytes(), gpu_lib.BOW_SEARCH_STATS_DTYPE)
    bow.close()
    mt.close()
    for p, (ikf, i_f) in enumerate(bc.PAIRS):
        kf, f = dict(sides[ikf], has_point=None), sides[i_f]
        want_n, want = bc.oracle_search(ob, kf, f, 0.7, 1)
        assert np.array_equal(match[p, :len(want)], want) and (match[p, len(want):] == -1).all() and stats["n_matches"][p] == want_n
