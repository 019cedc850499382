"""CPU: the plain-Python restatement of DBoW2's transform (tests/bow_restatement.py) against independent numpy properties and a hand tree
with every value written out; the vocabulary checks of amos_bow_create through the C ABI (no device is touched); the host-only text
parser of the C++ drop-in."""
import ctypes as C

import numpy as np
import pytest

import bow_restatement as br

_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)


def _np_dist(f, descs):
    return _POP[np.bitwise_xor(descs, f[None, :])].sum(1)


CASES = [dict(k=4, L=3, seed=1), dict(k=3, L=4, seed=2, duplicate_share=0.5), dict(k=5, L=3, seed=3, irregular=True),
         dict(k=1, L=4, seed=4), dict(k=6, L=1, seed=5)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"k{c['k']}L{c['L']}")
@pytest.mark.parametrize("levelsup", ["0", "4", "L", "L+1"])
def test_restatement_properties(case, levelsup):
    voc = br.make_vocabulary(**case)
    lu = {"0": 0, "4": 4, "L": voc.L, "L+1": voc.L + 1}[levelsup]
    feats = br.make_features(voc, 60, seed=case["seed"] + 100)
    r = br.transform(voc, feats, lu)
    depth = np.zeros(voc.n_nodes, int)
    for nid in range(1, voc.n_nodes):
        depth[nid] = depth[voc.parent[nid]] + 1
    kept = []
    for i, f in enumerate(feats):
        wid, w, nid, early, path = br.transform_feature(voc, f, lu)
        # each step's chosen child is the argmin with the lowest position (numpy's argmin returns the first minimum)
        for nodes, dists, chosen in path:
            d = _np_dist(f, voc.desc[np.array(nodes)])
            assert list(d) == dists and chosen == nodes[int(np.argmin(d))]
            assert nodes == [n for n in range(voc.n_nodes) if n > 0 and voc.parent[n] == voc.parent[nodes[0]]]  # ascending ids
        leaf = path[-1][2]
        assert voc.is_leaf[leaf] and all(not voc.is_leaf[p[2]] for p in path[:-1])
        # nid: the walk's node at level L - levelsup, the root at or below level 0, the leaf when the walk ends above the level
        level = voc.L - lu
        if level <= 0:
            assert nid == 0 and not early
        elif level <= len(path):
            assert nid == path[level - 1][2] and depth[nid] == level and not early
        else:
            assert nid == leaf and early
        assert r["feat_node"][i] == nid
        assert r["feat_word"][i] == (wid if w > 0 else br.NO_WORD)
        if w > 0:
            kept.append(i)
    # the FeatureVector partitions exactly the features that are not stopped, ids and indices ascending
    ids, off, idx = r["node_ids"], r["node_off"], r["node_idx"]
    assert np.all(np.diff(ids.astype(np.int64)) > 0) and off[0] == 0 and off[-1] == len(idx) and np.all(np.diff(off) > 0)
    assert sorted(idx.tolist()) == kept
    for a in range(len(ids)):
        seg = idx[off[a]:off[a + 1]]
        assert np.all(np.diff(seg) > 0) and np.all(r["feat_node"][seg] == ids[a])
    # the BowVector: ascending words, exactly the words of the kept features, summing to 1 within n * 2^-52
    words, wts = r["words"], r["word_weights"]
    assert np.all(np.diff(words.astype(np.int64)) > 0) and set(words.tolist()) == {int(r["feat_word"][i]) for i in kept}
    if len(kept):
        assert abs(float(np.sum(wts)) - 1.0) <= len(words) * 2.0 ** -52 and np.all(wts > 0)
    assert r["stats"]["n_stopped"] == len(feats) - len(kept) and r["stats"]["n_words"] == len(words) and r["stats"]["n_nodes"] == len(ids)
    assert (r["stats"]["status"] == 1) == any(br.transform_feature(voc, f, lu)[3] for f in feats)


def _hand_tree():
    """Seven nodes: root 0 -> 1, 2; 1 -> 3 (leaf, word 0), 4 (leaf, word 1); 2 -> 5 (leaf, word 2), 6 (leaf, word 3, stopped)."""
    d = np.zeros((7, 32), np.uint8)
    d[1, 0] = 0x00; d[2, 0] = 0xFF
    d[3, 1] = 0x00; d[4, 1] = 0x0F
    d[5, 1] = 0x00; d[6, 1] = 0xFF
    d[5, 0] = d[6, 0] = 0xFF
    return br.Vocabulary(2, 2, [0, 0, 0, 1, 1, 2, 2], [0, 0, 0, 1, 1, 1, 1], d, [0, 0, 0, 0.5, 1.5, 2.0, 0.0])


def test_hand_tree_every_value():
    voc = _hand_tree()
    assert voc.children == [[1, 2], [3, 4], [5, 6], [], [], [], []] and voc.word_id == [None, None, None, 0, 1, 2, 3]
    f = np.zeros((6, 32), np.uint8)
    f[0, 0], f[0, 1] = 0x00, 0x00  # -> 1 -> 3: word 0 (0.5)
    f[1, 0], f[1, 1] = 0x01, 0x0F  # -> 1 -> 4: word 1 (1.5)
    f[2, 0], f[2, 1] = 0xFF, 0x00  # -> 2 -> 5: word 2 (2.0)
    f[3, 0], f[3, 1] = 0xFE, 0xFF  # -> 2 -> 6: word 3, weight 0: stopped
    f[4, 0], f[4, 1] = 0x0F, 0x03  # ties at both levels (4 : 4 and 2 : 2): the first child -> 1 -> 3: word 0
    f[5, 0], f[5, 1] = 0x00, 0x1F  # -> 1 -> 4: word 1
    r = br.transform(voc, f, 1)  # nid at level 1
    assert r["feat_word"].tolist() == [0, 1, 2, br.NO_WORD, 0, 1]
    assert r["feat_node"].tolist() == [1, 1, 2, 2, 1, 1]
    assert r["fv"] == {1: [0, 1, 4, 5], 2: [2]}
    assert r["node_ids"].tolist() == [1, 2] and r["node_off"].tolist() == [0, 4, 5] and r["node_idx"].tolist() == [0, 1, 4, 5, 2]
    # values 0.5 + 0.5 = 1, 1.5 + 1.5 = 3, 2; norm 6
    assert r["words"].tolist() == [0, 1, 2] and r["word_weights"].tolist() == [1.0 / 6.0, 3.0 / 6.0, 2.0 / 6.0]
    assert r["stats"] == {"n_words": 3, "n_nodes": 2, "n_stopped": 1, "status": 0}
    assert br.transform(voc, f, 0)["feat_node"].tolist() == [3, 4, 5, 6, 3, 4]  # the leaves
    assert br.transform(voc, f, 2)["feat_node"].tolist() == [0] * 6 and br.transform(voc, f, 3)["fv"] == {0: [0, 1, 2, 4, 5]}


def test_search_restatement_equals_the_oracle(ob):
    """The Python SearchByBoW against orc_search_by_bow on random clustered descriptors: matches and the return value."""
    import bow_search_cases as bc
    for seed in range(4):
        kf, f = bc.random_pair(seed, n_kf=90, n_f=110, n_nodes=6, has_point_share=0.8 if seed % 2 else None)
        for ori in (0, 1):
            want_n, want = bc.oracle_search(ob, kf, f, 0.75, ori)
            got, stats = br.search_by_bow(kf, f, 0.75, ori)
            assert got.tolist() == want.tolist() and stats["n_matches"] == want_n


def test_search_inputs_meet_their_conditions(ob, synth):
    """What tests/test_gpu_bow_search.py relies on, checked with the oracle (and its replay) alone: every large case has at least 30
    matches, and keyframe features whose unrestricted best two were already matched do occur."""
    import bow_search_cases as bc
    for nodes in sorted(bc.NODE_LEVELS):
        sides = bc.synth_sides(ob, synth, "large", nodes)
        assert abs(len(sides[0]["fv"]) - int(nodes)) <= int(nodes) // 5  # about 100 / about 10 nodes
        researched = 0
        for with_has_point in (False, True):
            for ikf, i_f in bc.PAIRS:
                kf = sides[ikf] if with_has_point else dict(sides[ikf], has_point=None)
                want_n, want = bc.oracle_search(ob, kf, sides[i_f], 0.7, 1)
                got, stats = br.search_by_bow(kf, sides[i_f], 0.7, 1)
                assert want_n >= 30 and got.tolist() == want.tolist() and stats["n_matches"] == want_n
                researched += stats["n_researched"]
        assert researched > 0


# ---- the vocabulary checks of amos_bow_create, before the device is touched

def _create(pkg, k, L, scoring, weighting, parent, is_leaf, desc=None, weight=None):
    parent, is_leaf = np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(is_leaf, np.uint8)
    n = len(parent)
    desc = np.zeros((n, 32), np.uint8) if desc is None else desc
    weight = np.ones(n, np.float64) if weight is None else weight
    h = C.c_void_p()
    rc = pkg.lib().amos_bow_create(0, None, k, L, scoring, weighting, n, pkg._p(parent), pkg._p(is_leaf), pkg._p(desc), pkg._p(weight), C.byref(h))
    assert h.value is None or rc == 0
    return rc


GOOD = dict(k=2, L=2, scoring=0, weighting=0, parent=[0, 0, 0, 1, 1, 2, 2], is_leaf=[0, 0, 0, 1, 1, 1, 1])
BAD = {
    "scoring": dict(GOOD, scoring=1),
    "weighting": dict(GOOD, weighting=1),
    "L0": dict(GOOD, L=0),
    "L11": dict(GOOD, L=11),
    "parent_self": dict(GOOD, parent=[0, 0, 2, 1, 1, 2, 2]),
    "parent_later": dict(GOOD, parent=[0, 0, 0, 1, 5, 2, 2]),
    "parent_negative": dict(GOOD, parent=[0, 0, 0, 1, -1, 2, 2]),
    "inner_without_children": dict(GOOD, is_leaf=[0, 0, 0, 1, 1, 1, 0]),
    "leaf_with_children": dict(GOOD, is_leaf=[0, 1, 0, 1, 1, 1, 1]),
    "33_children": dict(GOOD, parent=[0] * 34, is_leaf=[0] + [1] * 33),
    "root_alone": dict(GOOD, parent=[0], is_leaf=[0]),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_create_rejects_before_the_device(pkg, name):
    c = BAD[name]
    assert _create(pkg, **c) == -1, pkg.lib().amos_last_error()
    assert pkg.bow_check(c["k"], c["L"], c["scoring"], c["weighting"], c["parent"], c["is_leaf"])[0] == -1
    assert pkg.lib().amos_last_error().decode().startswith("amos_bow_check")


def test_check_accepts_and_counts_words(pkg):
    assert pkg.bow_check(GOOD["k"], GOOD["L"], 0, 0, GOOD["parent"], GOOD["is_leaf"]) == (0, 4)
    assert pkg.bow_check(32, 1, 0, 0, [0] * 33, [0] + [1] * 32) == (0, 32)  # 32 children are the most
    voc = br.make_vocabulary(5, 3, seed=7, irregular=True)
    assert pkg.bow_check(voc.k, voc.L, 0, 0, voc.parent, voc.is_leaf) == (0, voc.n_words)
    h = C.c_void_p()
    assert pkg.lib().amos_bow_create(0, None, 2, 2, 0, 0, 7, None, None, None, None, C.byref(h)) == -1  # NULL arrays
    lib = pkg.lib()
    z = np.zeros(8, np.uint8)
    assert lib.amos_bow_transform_batch_device(None, pkg._p(z), pkg._p(z), 1, 8, 4, *([pkg._p(z)] * 10)) == -1
    assert lib.amos_match_bow_batch_device(None, None) == -1 and lib.amos_match_bow(None, None, None, 0.7, 1, None, None) == -1


# ---- the text loader of the C++ drop-in (ORB_SLAM2::DeviceVocabulary::loadFromTextFile): host only

def test_text_parser_round_trip(tmp_path):
    import host_bow_binding as hbb
    voc = br.make_vocabulary(4, 3, seed=9, irregular=True)
    path = tmp_path / "voc.txt"
    path.write_text(voc.to_text() + "\n")  # (a trailing empty line is skipped)
    v = hbb.Vocabulary(path)
    assert v.status == 0 and v.h, v.error
    a = v.arrays()
    assert (a["k"], a["L"], a["scoring"], a["weighting"], a["nodes"], a["words"]) == (4, 3, 0, 0, voc.n_nodes, voc.n_words)
    assert np.array_equal(a["parent"][1:], voc.parent[1:]) and np.array_equal(a["is_leaf"][1:], voc.is_leaf[1:])
    assert np.array_equal(a["desc"][1:], voc.desc[1:]) and a["weight"][1:].tobytes() == voc.weight[1:].tobytes()  # repr round-trips a double
    v.close()


def _lines(voc):
    return voc.to_text().splitlines()


MALFORMED = {
    "missing_file": None,
    "empty_file": lambda L: [],
    "header_three_numbers": lambda L: ["4 3 0"] + L[1:],
    "header_text": lambda L: ["k L 0 0"] + L[1:],
    "scoring_not_l1": lambda L: ["4 3 1 0"] + L[1:],
    "weighting_not_tf_idf": lambda L: ["4 3 0 2"] + L[1:],
    "L_out_of_range": lambda L: ["4 11 0 0"] + L[1:],
    "short_descriptor": lambda L: L[:3] + [" ".join(L[3].split()[:-2])] + L[4:],
    "byte_256": lambda L: L[:3] + [" ".join(L[3].split()[:5] + ["256"] + L[3].split()[6:])] + L[4:],
    "extra_field": lambda L: L[:3] + [L[3] + " 1.0"] + L[4:],
    "text_in_a_node": lambda L: L[:3] + [L[3].replace(L[3].split()[4], "x", 1)] + L[4:],
    "parent_ahead": lambda L: L[:2] + ["9 " + L[2].split(" ", 1)[1]] + L[3:],
    "only_the_header": lambda L: L[:1],
    "leaf_with_children": lambda L: [L[0], "0 1 " + L[1].split(" ", 2)[2]] + ["1 1 " + L[2].split(" ", 2)[2]],
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_text_parser_rejects_malformed_input(tmp_path, name):
    import host_bow_binding as hbb
    path = tmp_path / "voc.txt"
    if MALFORMED[name] is not None:
        lines = MALFORMED[name](_lines(br.make_vocabulary(4, 3, seed=9)))
        path.write_text("".join(line + "\n" for line in lines))
    v = hbb.Vocabulary(path)
    assert v.status == -1 and not v.h and v.error, name  # AMOS_ERR_INVALID
