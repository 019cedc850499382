"""amos_bow_transform_batch_device / amos_bow_transform on the GPU against the plain-Python restatement of DBoW2's transform
(tests/bow_restatement.py), bit for bit: every per-feature output, the FeatureVector's CSR, the BowVector with its doubles as bytes, every
stat, and the padding of every array, poisoned beforehand and found intact."""
import functools

import numpy as np
import pytest

import bow_restatement as br

pytestmark = pytest.mark.gpu

POISON = 0xA5
# name -> (make_vocabulary arguments, levelsup)
TREES = {
    "k10L3": (dict(k=10, L=3, seed=11), 1),                        # 1 110 nodes
    "k3L6": (dict(k=3, L=6, seed=12), 4),                          # 1 093 nodes; ORB-SLAM2's levelsup
    "k20L2": (dict(k=20, L=2, seed=13), 1),                        # the second round of the descent: children 17 .. 20
    "chain": (dict(k=1, L=5, seed=14, bad_weight_share=0.0), 2),   # one child per node
    "k32L1": (dict(k=32, L=1, seed=15), 0),                        # the most children
    "irregular6": (dict(k=6, L=5, seed=16, irregular=True), 0),    # leaves above level L - levelsup: status bit 0
    "irregular20": (dict(k=20, L=3, seed=17, irregular=True, duplicate_share=0.3), 1),
}
COUNTS = [0, 1, 3, 4, 5, 63, 64, 65, 1000]


@functools.lru_cache(maxsize=None)
def tree(name):
    return br.make_vocabulary(**TREES[name][0])


@functools.lru_cache(maxsize=None)
def features(name):
    return br.make_features(tree(name), 1000, seed=sum(map(ord, name)))


@functools.lru_cache(maxsize=None)
def reference(name, n, levelsup):
    return br.transform(tree(name), features(name)[:n], levelsup)


@pytest.fixture(scope="module")
def handles(gpu_lib):
    made = {}

    def get(name):
        if name not in made:
            v = tree(name)
            made[name] = gpu_lib.BowVocabulary(v.k, v.L, *v.arrays())
        return made[name]
    yield get
    for h in made.values():
        h.close()


class Outputs:
    """the device arrays of one call, poisoned"""

    def __init__(self, nf, cap):
        import torch

        def buf(rows, width):
            return torch.full((rows, width), POISON, dtype=torch.uint8, device="cuda")
        self.nf, self.cap = nf, cap
        self.t = dict(feat_word=buf(nf, cap * 4), feat_node=buf(nf, cap * 4), n_nodes=buf(nf, 4), node_ids=buf(nf, cap * 4),
                      node_off=buf(nf, (cap + 1) * 4), node_idx=buf(nf, cap * 4), n_words=buf(nf, 4), words=buf(nf, cap * 4),
                      word_weights=buf(nf, cap * 8), stats=buf(nf, 16))

    def ptrs(self):
        return [self.t[k].data_ptr() for k in ("feat_word", "feat_node", "n_nodes", "node_ids", "node_off", "node_idx", "n_words", "words",
                                               "word_weights", "stats")]

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def upload(frames, cap):
    import torch
    desc = np.full((len(frames), cap, 32), 0x5A, np.uint8)
    for f, d in enumerate(frames):
        desc[f, :len(d)] = d
    counts = np.array([len(d) for d in frames], np.int32)
    return torch.from_numpy(desc).cuda(), torch.from_numpy(counts).cuda()


def run_batch(handle, frames, levelsup, cap):
    import torch
    d_desc, d_counts = upload(frames, cap)
    out = Outputs(len(frames), cap)
    torch.cuda.synchronize()
    handle.transform_batch_device(d_desc.data_ptr(), d_counts.data_ptr(), len(frames), cap, levelsup, *out.ptrs())
    handle.sync()
    return out.host()


def check_frame(pkg, got, f, want, n):
    """row f of every output == the restatement's arrays, and the rest of the row is still poison"""
    st = np.frombuffer(got["stats"][f].tobytes(), pkg.BOW_STATS_DTYPE)[0]
    ws = want["stats"]
    print(f"frame {f}: {n} features, words {st['n_words']} / {ws['n_words']}, nodes {st['n_nodes']} / {ws['n_nodes']}, stopped "
          f"{st['n_stopped']} / {ws['n_stopped']}, status {st['status']} / {ws['status']}")
    assert {k: int(st[k]) for k in ws} == ws
    nn, nw, m = ws["n_nodes"], ws["n_words"], n - ws["n_stopped"]
    assert np.frombuffer(got["n_nodes"][f].tobytes(), np.int32)[0] == nn and np.frombuffer(got["n_words"][f].tobytes(), np.int32)[0] == nw
    for name, arr, cnt in (("feat_word", want["feat_word"], n), ("feat_node", want["feat_node"], n), ("node_ids", want["node_ids"], nn),
                           ("node_off", want["node_off"], nn + 1), ("node_idx", want["node_idx"], m), ("words", want["words"], nw),
                           ("word_weights", want["word_weights"], nw)):
        assert len(arr) == cnt, name
        row, nbytes = got[name][f], cnt * arr.dtype.itemsize
        assert row[:nbytes].tobytes() == arr.tobytes(), name
        assert (row[nbytes:] == POISON).all(), name + " padding"


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", sorted(TREES))
def test_one_frame(gpu_lib, handles, name, n):
    lu = TREES[name][1]
    got = run_batch(handles(name), [features(name)[:n]], lu, cap=n + 3)
    check_frame(gpu_lib, got, 0, reference(name, n, lu), n)


@pytest.mark.parametrize("name", sorted(TREES))
def test_three_frames_with_different_counts(gpu_lib, handles, name):
    lu = TREES[name][1]
    counts = [65, 0, 1000]
    got = run_batch(handles(name), [features(name)[:n] for n in counts], lu, cap=1000)  # the last frame fills its row
    for f, n in enumerate(counts):
        check_frame(gpu_lib, got, f, reference(name, n, lu), n)
    # the irregular trees, and only they, show the early-leaf bit
    assert reference(name, 1000, lu)["stats"]["status"] == (1 if name.startswith("irregular") else 0)


@pytest.mark.parametrize("levelsup", [0, 2, 3, 4, 9])
def test_levelsup(gpu_lib, handles, levelsup):
    """nid at the leaves, inside the tree, at level 0 and below it (k10L3: L - levelsup = 3, 1, 0, -1, -6)"""
    got = run_batch(handles("k10L3"), [features("k10L3")[:65]], levelsup, cap=70)
    check_frame(gpu_lib, got, 0, reference("k10L3", 65, levelsup), 65)
    got = run_batch(handles("irregular6"), [features("irregular6")[:65]], levelsup, cap=70)
    check_frame(gpu_lib, got, 0, reference("irregular6", 65, levelsup), 65)


def test_all_words_stopped(gpu_lib):
    voc = br.make_vocabulary(4, 3, seed=21, all_stopped=True)
    feats = br.make_features(voc, 70, seed=22)
    want = br.transform(voc, feats, 1)
    assert want["stats"] == {"n_words": 0, "n_nodes": 0, "n_stopped": 70, "status": 0} and want["node_off"].tolist() == [0]
    h = gpu_lib.BowVocabulary(voc.k, voc.L, *voc.arrays())
    check_frame(gpu_lib, run_batch(h, [feats], 1, cap=72), 0, want, 70)
    h.close()


def test_duplicates_among_siblings(gpu_lib):
    """every second child copies its elder sibling: the first of equal distances wins at every level; features that ARE node descriptors"""
    voc = br.make_vocabulary(8, 3, seed=23, duplicate_share=0.6, bad_weight_share=0.0)
    rng = np.random.default_rng(24)
    feats = voc.desc[rng.integers(1, voc.n_nodes, 200)].copy()
    want = br.transform(voc, feats, 1)
    ties = sum(1 for f in feats for nodes, dists, chosen in br.transform_feature(voc, f, 1)[4] if dists.count(min(dists)) > 1)
    assert ties >= 50, ties
    h = gpu_lib.BowVocabulary(voc.k, voc.L, *voc.arrays())
    check_frame(gpu_lib, run_batch(h, [feats], 1, cap=200), 0, want, 200)
    h.close()


def test_handle_used_twice_without_a_sync_between(gpu_lib, handles):
    import torch
    h, name = handles("k3L6"), "k3L6"
    calls = []
    for n, cap in ((1000, 1000), (63, 80)):  # the second call is smaller: the scratch of the first is reused
        d_desc, d_counts = upload([features(name)[:n]], cap)
        out = Outputs(1, cap)
        calls.append((n, d_desc, d_counts, out))
    torch.cuda.synchronize()
    for n, d_desc, d_counts, out in calls:
        h.transform_batch_device(d_desc.data_ptr(), d_counts.data_ptr(), 1, out.cap, 4, *out.ptrs())
    h.sync()
    for n, _, _, out in calls:
        check_frame(gpu_lib, out.host(), 0, reference(name, n, 4), n)


@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_host_form_equals_batch_form(gpu_lib, handles, n):
    name, lu = "k10L3", 1
    want = reference(name, n, lu)
    got = handles(name).transform(features(name)[:n], lu)
    assert {k: int(got["stats"][k]) for k in want["stats"]} == want["stats"]
    for k in ("feat_word", "feat_node", "node_ids", "node_off", "node_idx", "words", "word_weights"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def test_largest_capacity_and_the_bound(gpu_lib, handles):
    """capacity 16 384 (the sort's 128 KB of LDS) runs; one more is AMOS_ERR_CAPACITY before anything is launched"""
    name, lu = "k10L3", 1
    got = run_batch(handles(name), [features(name)[:1000]], lu, cap=gpu_lib.BOW_MAX_CAPACITY)
    check_frame(gpu_lib, got, 0, reference(name, 1000, lu), 1000)
    with pytest.raises(gpu_lib.AmosError, match="rc=-3"):
        run_batch(handles(name), [features(name)[:5]], lu, cap=gpu_lib.BOW_MAX_CAPACITY + 1)
