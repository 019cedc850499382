"""amos_match_fuse_batch_device / amos_match_fuse on the GPU against the restatement (tests/fuse_restatement.py), bit for bit: u, v, ur and
level of d_query, d_in_view, d_best_idx, d_best_dist and d_stats.  tests/test_fuse_cpu.py holds the restatement to the oracle and asserts that
the shared scene contains every case (pre-filter exits, borders, wide windows, both chi-square constants, ties, the threshold)."""
import numpy as np
import pytest

import fuse_restatement as fr
import local_points_restatement as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    return fr.scene()


@pytest.fixture(scope="module")
def want(sc):
    """the restatement, once per (mode, stereo) and pair subset"""
    cache = {}

    def get(mode, with_right, pairs=None):
        key = (mode, with_right, None if pairs is None else tuple(pairs))
        if key not in cache:
            sel = sc["pairs"] if pairs is None else [sc["pairs"][p] for p in pairs]
            cache[key] = fr.fuse(sc["kfs"], sc["points"], sel, sc["skip"], sc["n_out"], sc["sf"], sc["inv_sigma2"], sc["bounds"], mode,
                                 with_right=with_right)
        return cache[key]
    return get


def compare(sc, pairs, got, w):
    query, in_view, best_idx, best_dist, stats = got
    owned = np.zeros(sc["n_out"], bool)
    for p, (frame, first, count, off, cam) in enumerate(pairs):
        s = slice(off, off + count)
        owned[s] = True
        print(f"pair {p}: {count} points, in view {w['stats'][p][0]} / {stats['n_in_view'][p]}, accepted {w['stats'][p][1]} / {stats['n_accepted'][p]}")
        assert np.array_equal(in_view[s], w["in_view"][s]), p
        for name in ("u", "v", "ur", "level", "src", "desc"):
            assert query[name][s].tobytes() == w["query"][name][s].tobytes(), (p, name)
        assert np.array_equal(best_idx[s], w["best_idx"][s]), p
        assert np.array_equal(best_dist[s], w["best_dist"][s]), p
        assert (stats["n_in_view"][p], stats["n_accepted"][p]) == tuple(w["stats"][p]), p
    return owned


class Resident:
    """the scene's keyframes and points uploaded once: capacity above every count, poison behind the counts"""

    def __init__(self, pkg, sc, pad=9, stream=None):
        import torch
        self.torch, self.pkg, self.sc = torch, pkg, sc
        kfs = sc["kfs"]
        nf = len(kfs)
        self.cap = cap = max(len(k) for k, _, _ in kfs) + pad
        rng = np.random.default_rng(5)
        kps = np.frombuffer(rng.integers(0, 256, nf * cap * pkg.KP_DTYPE.itemsize, dtype=np.uint8).tobytes(), pkg.KP_DTYPE).reshape(nf, cap).copy()
        kps["x"], kps["y"], kps["octave"] = 100.0, 100.0, 1  # poison that WOULD be a candidate if an index past a count were read
        desc = np.full((nf, cap, 32), 0xFF, np.uint8)
        ur, cell, counts = np.full((nf, cap), 50.0, np.float32), np.full((nf, cap), 7 * 48 + 3, np.int32), np.zeros(nf, np.int32)
        for f, (k, d, r) in enumerate(kfs):
            n = counts[f] = len(k)
            kps[f, :n], desc[f, :n], ur[f, :n] = k, d, r
            cell[f, :n] = lr.grid_cells(k, sc["bounds"])
        up = self.up
        self.d_kps, self.d_desc, self.d_ur, self.d_cell, self.d_counts = up(kps), up(desc), up(ur), up(cell), up(counts)
        self.d_points, self.d_skip = up(sc["points"]), up(sc["skip"])
        self.d_start = torch.zeros((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
        self.d_items = torch.full((nf, cap), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.mt = pkg.OrbMatcher(stream=stream)
        self.mt.grid_build_batch_device(self.d_cell.data_ptr(), self.d_counts.data_ptr(), nf, cap, self.d_start.data_ptr(), self.d_items.data_ptr())
        self.mt.sync()

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def alloc(self, n_pairs):
        """poisoned outputs"""
        torch, n_out = self.torch, self.sc["n_out"]
        b = dict(query=torch.full((n_out, 52), 0xEE, dtype=torch.uint8, device="cuda"), in_view=torch.full((n_out,), 7, dtype=torch.uint8, device="cuda"),
                 idx=torch.full((n_out,), 12345, dtype=torch.int32, device="cuda"), dist=torch.full((n_out,), 12345, dtype=torch.int32, device="cuda"),
                 stats=torch.full((max(n_pairs, 1), 2), -9, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        return b

    def launch(self, b, pairs, mode, with_right, over=None):
        """the batch call alone (asynchronous)"""
        sc = self.sc
        a = dict(d_kps=self.d_kps.data_ptr(), d_desc=self.d_desc.data_ptr(), d_counts=self.d_counts.data_ptr(), d_cell_start=self.d_start.data_ptr(),
                 d_items=self.d_items.data_ptr(), d_points=self.d_points.data_ptr(), n_points=len(sc["points"]), n_frames=len(sc["kfs"]),
                 pair_frame=[p[0] for p in pairs], point_first=[p[1] for p in pairs], point_count=[p[2] for p in pairs],
                 out_off=[p[3] for p in pairs], cameras=np.array([p[4] for p in pairs], fr.CAMERA), capacity=self.cap, scale_factors=sc["sf"],
                 inv_level_sigma2=sc["inv_sigma2"], d_query=b["query"].data_ptr(), d_in_view=b["in_view"].data_ptr(), d_best_idx=b["idx"].data_ptr(),
                 d_best_dist=b["dist"].data_ptr(), d_stats=b["stats"].data_ptr(), mode=mode, max_dist=50, bounds=sc["bounds"],
                 d_u_right=self.d_ur.data_ptr() if with_right else None, d_skip=self.d_skip.data_ptr())
        a.update(over or {})
        self.mt.fuse_batch_device(**a)

    def fetch(self, b):
        self.mt.sync()
        self.torch.cuda.synchronize()
        query = np.frombuffer(b["query"].cpu().numpy().tobytes(), self.pkg.WINDOW_QUERY_DTYPE)
        stats = np.frombuffer(b["stats"].cpu().numpy().tobytes(), self.pkg.FUSE_STATS_DTYPE)
        return query, b["in_view"].cpu().numpy(), b["idx"].cpu().numpy(), b["dist"].cpu().numpy(), stats

    def run(self, pairs, mode, with_right, over=None):
        """one batch call -> (query, in_view, best_idx, best_dist, stats); outputs start poisoned"""
        b = self.alloc(len(pairs))
        self.launch(b, pairs, mode, with_right, over)
        return self.fetch(b)


@pytest.fixture(scope="module")
def resident(gpu_lib, sc):
    r = Resident(gpu_lib, sc)
    yield r
    r.mt.close()


@pytest.mark.parametrize("mode", [fr.LOCAL, fr.SIM3])
@pytest.mark.parametrize("with_right", [True, False])
def test_batch_entry_against_the_restatement(resident, sc, want, mode, with_right):
    got = resident.run(sc["pairs"], mode, with_right)
    owned = compare(sc, sc["pairs"], got, want(mode, with_right))
    query, in_view, best_idx, best_dist, _ = got
    # entries no pair owns keep what they held
    assert (in_view[~owned] == 7).all() and (best_idx[~owned] == 12345).all() and (best_dist[~owned] == 12345).all()
    assert (query.view(np.uint8).reshape(-1, 52)[~owned] == 0xEE).all()


def test_second_call_with_fewer_pairs_and_points(resident, sc, want):
    """one handle: the whole scene, then two of its smaller pairs -- per-pair parameters or counts left over from the first call would show"""
    resident.run(sc["pairs"], fr.LOCAL, True)
    few = [2, 4]
    pairs = [sc["pairs"][p] for p in few]
    got = resident.run(pairs, fr.LOCAL, True)
    owned = compare(sc, pairs, got, want(fr.LOCAL, True, few))
    assert (got[1][~owned] == 7).all() and (got[2][~owned] == 12345).all()


@pytest.mark.parametrize("mode,with_right", [(fr.LOCAL, True), (fr.LOCAL, False), (fr.SIM3, True)])
def test_host_form_against_the_restatement(gpu_lib, sc, want, mode, with_right):
    mt = gpu_lib.OrbMatcher()
    kfs = [dict(keys_un=k, desc=d, u_right=r if with_right and f != 2 else None) for f, (k, d, r) in enumerate(sc["kfs"])]
    if with_right:  # keyframe 2 is monocular among stereo ones: its u_right is all -1
        kf2 = sc["kfs"][2]
        scene_kfs = list(sc["kfs"])
        scene_kfs[2] = (kf2[0], kf2[1], np.full(len(kf2[0]), -1, np.float32))
        w = fr.fuse(scene_kfs, sc["points"], sc["pairs"], sc["skip"], sc["n_out"], sc["sf"], sc["inv_sigma2"], sc["bounds"], mode)
    else:
        w = want(mode, False)

    def call(pairs):
        return mt.fuse(kfs, sc["points"], [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], [p[3] for p in pairs],
                       np.array([p[4] for p in pairs], fr.CAMERA), sc["sf"], sc["inv_sigma2"], sc["n_out"], skip=sc["skip"], mode=mode,
                       bounds=sc["bounds"])
    got = call(sc["pairs"])
    owned = compare(sc, sc["pairs"], got, w)
    assert (got[1][~owned] == 0).all() and (got[2][~owned] == -1).all() and (got[3][~owned] == 256).all()
    few = [sc["pairs"][p] for p in (1, 3)]  # the same handle again, smaller
    w2 = fr.fuse([(k["keys_un"], k["desc"], k["u_right"]) for k in kfs] if not with_right else scene_kfs, sc["points"], few, sc["skip"], sc["n_out"],
                 sc["sf"], sc["inv_sigma2"], sc["bounds"], mode, with_right=with_right)
    compare(sc, few, call(few), w2)
    # no keyframes and no pairs, and keyframes without pairs, are valid and compute nothing
    q, iv, bi, bd, st = mt.fuse([], sc["points"], [], [], [], [], np.zeros(0, fr.CAMERA), sc["sf"], sc["inv_sigma2"], 4, mode=mode, bounds=sc["bounds"])
    assert (bi == -1).all() and len(st) == 0
    mt.close()


def test_invalid_arguments(resident, sc, gpu_lib):
    pairs = [sc["pairs"][2], sc["pairs"][4]]
    ok = resident.run(pairs, fr.LOCAL, True)
    assert ok[4]["n_accepted"][0] > 0
    bad = [dict(d_kps=None), dict(d_points=None), dict(d_query=None), dict(d_stats=None), dict(d_best_idx=None), dict(inv_level_sigma2=None),
           dict(pair_frame=[1, 4]), dict(pair_frame=[-1, 2]), dict(point_first=[-1, 0]), dict(point_count=[31, len(sc["points"]) + 1]),
           dict(out_off=[pairs[1][3], pairs[0][3]]), dict(out_off=[10, 20]), dict(capacity=0), dict(capacity=65537),
           dict(scale_factors=np.ones(17, np.float32), inv_level_sigma2=np.ones(17, np.float32)), dict(bounds=(0.0, 0.0, 0.0, 480.0)),
           dict(bounds=(0.0, 640.0, 5.0, 5.0)), dict(mode=2), dict(n_frames=0)]
    for over in bad:
        with pytest.raises(gpu_lib.AmosError) as e:
            resident.run(pairs, fr.LOCAL, True, over)
        assert "amos_match_fuse_batch_device" in str(e.value), over
    resident.run(pairs, fr.SIM3, True, dict(inv_level_sigma2=None))  # the table is read in the local mode only
    again = resident.run(pairs, fr.LOCAL, True)                # and the handle still works
    assert all(np.array_equal(a, b) for a, b in zip(ok[1:4], again[1:4]))
