"""amos_match_sim3_optimize_batch_device on the GPU against the restatement (tests/sim3_optimization_restatement.py), with == on whole rows
and on the raw bytes of the result records.  One batch call holds the grid of tests/sim3_optimization_cases.py (every correspondence count,
both fix_scale values, 0 % and 25 % gross outliers), eight pairs that share keyframe slot 0 of their own, a disabled pair and two pairs
with a slot outside the frames; it runs with separate row arrays and in place, and capacity is larger than every count.  Outputs start
poisoned so that "not written" is visible, and what lies behind a keyframe's count would change the result if it were read."""
import numpy as np
import pytest

import sim3_optimization_cases as sc
import sim3_optimization_restatement as so
import sim3_search_restatement as ss

pytestmark = pytest.mark.gpu
f32 = np.float32
OUT_POISON, CAP = 12345, 448
SEARCH_POISON = 12345


def candidates():
    """eight candidates for one current keyframe: keyframe 2 of one scene with other observations, rows and start Sim3s"""
    base = sc.scene(64, 0, 0.25, seed=7)
    rng = np.random.default_rng(70)
    out = []
    for k in range(8):
        s = dict(base)
        s["kps2"] = base["kps2"].copy()
        s["kps2"]["x"] += rng.uniform(-0.5, 0.5, len(s["kps2"])).astype(np.float32)
        s["kps2"]["y"] += rng.uniform(-0.5, 0.5, len(s["kps2"])).astype(np.float32)
        s["row"] = base["row"].copy()
        s["row"][rng.permutation(len(s["row"]))[:4 * k]] = -1
        p = base["pair"].copy()
        p["t12"] += rng.uniform(-0.01, 0.01, 3).astype(np.float32)
        p["fix_scale"] = k & 1
        s["pair"] = p
        out.append(s)
    return out


class Batch:
    """frames: per grid scene keyframe 1 and keyframe 2; then the shared keyframe 1 and its eight candidates"""

    def __init__(self):
        grid, want = sc.shared()
        self.scenes = [s for _, s in grid]
        self.want = list(want)
        cands = candidates()
        self.want += [sc.expected(s) for s in cands]
        frames, self.slots = [], []
        for s in self.scenes:
            self.slots.append((len(frames), len(frames) + 1))
            frames += [(s["kps1"], s["pts1"], s["cam1"]), (s["kps2"], s["pts2"], s["cam2"])]
        shared_slot = len(frames)
        frames.append((cands[0]["kps1"], cands[0]["pts1"], cands[0]["cam1"]))
        for s in cands:
            self.slots.append((shared_slot, len(frames)))
            frames.append((s["kps2"], s["pts2"], s["cam2"]))
        self.scenes += cands
        self.nf = len(frames)
        self.kps, self.pts = np.zeros((self.nf, CAP), so.KP_DTYPE), np.zeros((self.nf, CAP), so.POINT)
        self.cams, self.counts = np.zeros(self.nf, so.CAMERA), np.zeros(self.nf, np.int32)
        self.kps["x"], self.kps["y"], self.kps["octave"] = 100.0, 100.0, 1  # poison that WOULD take part if an index past a count were read
        self.pts["pos"] = (0.0, 0.0, 3.0)
        for f, (k, p, c) in enumerate(frames):
            self.kps[f, :len(k)], self.pts[f, :len(k)], self.cams[f], self.counts[f] = k, p, c, len(k)
        self.rows = np.full((len(self.scenes), CAP), 5, np.int32)  # behind N1: entries that would be correspondences
        for p, s in enumerate(self.scenes):
            self.rows[p, :len(s["row"])] = s["row"]
        self.pairs = np.array([s["pair"] for s in self.scenes], so.PAIR)

    def want_arrays(self, which=None, wants=None):
        which = range(len(self.scenes)) if which is None else which
        wants = [self.want[p] for p in which] if wants is None else wants
        rows = self.rows[list(which)].copy()
        for k, (res, row) in enumerate(wants):
            rows[k, :len(row)] = row
        return rows, np.array([w[0] for w in wants], so.RESULT)


@pytest.fixture(scope="module")
def batch():
    return Batch()


class Resident:
    def __init__(self, pkg, b):
        import torch
        self.torch, self.pkg, self.b = torch, pkg, b
        self.d_kps, self.d_pts = self.up(b.kps), self.up(b.pts)
        self.mt = pkg.OrbMatcher()
        self.set_counts(b.counts)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def set_counts(self, counts):
        self.d_counts = self.up(np.asarray(counts, np.int32))

    def run(self, which=None, in_place=False, pairs=None, slots=None, sim3=None):
        """one batch call -> (rows out [pairs][CAP], result records [pairs])"""
        torch, b = self.torch, self.b
        which = list(range(len(b.scenes))) if which is None else list(which)
        n = len(which)
        pairs = b.pairs[which] if pairs is None else pairs
        slots = [b.slots[p] for p in which] if slots is None else slots
        d_rows = self.up(b.rows[which])
        d_out = d_rows if in_place else torch.full((n, CAP), OUT_POISON, dtype=torch.int32, device="cuda")
        d_res = torch.full((n, 256), 0x5A, dtype=torch.uint8, device="cuda")
        d_1, d_2 = self.up(np.array([s[0] for s in slots], np.int32)), self.up(np.array([s[1] for s in slots], np.int32))
        d_sim3 = None if sim3 is None else self.up(sim3)
        torch.cuda.synchronize()
        self.mt.sim3_optimize_batch_device(self.d_kps.data_ptr(), self.d_counts.data_ptr(), self.d_pts.data_ptr(), b.cams, d_1.data_ptr(), d_2.data_ptr(),
                                           pairs, d_rows.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), CAP, sc.INV_SIGMA2,
                                           d_sim3=None if d_sim3 is None else d_sim3.data_ptr())
        self.mt.sync()
        torch.cuda.synchronize()
        return (np.frombuffer(d_out.cpu().numpy().tobytes(), np.int32).reshape(n, CAP), np.frombuffer(d_res.cpu().numpy().tobytes(), so.RESULT))


@pytest.fixture(scope="module")
def res(gpu_lib, batch):
    return Resident(gpu_lib, batch)


def assert_equal(got, want, what):
    rows, recs = got
    wrows, wrecs = want
    assert np.array_equal(rows, wrows), (what, "rows", np.argwhere(rows != wrows)[:5].tolist())
    for p in range(len(wrecs)):
        if recs[p].tobytes() != wrecs[p].tobytes():
            diff = [f for f in so.RESULT.names if np.asarray(recs[p][f]).tobytes() != np.asarray(wrecs[p][f]).tobytes()]
            raise AssertionError((what, "record", p, diff, recs[p], wrecs[p]))


def special(b, n_frames):
    """the full batch with pair 1 disabled, pair 2 with keyframe 1's slot outside the frames and pair 5 with keyframe 2's"""
    pairs, slots = b.pairs.copy(), list(b.slots)
    pairs["enabled"][1] = 0
    pairs["th2"][1] = -1.0  # (a disabled pair's record is not looked into)
    slots[2], slots[5] = (n_frames, slots[2][1]), (slots[5][0], -1)
    return pairs, slots


@pytest.mark.parametrize("in_place", [False, True])
def test_batch_equals_the_restatement(batch, res, in_place):
    pairs, slots = special(batch, batch.nf)
    got = res.run(pairs=pairs, slots=slots, in_place=in_place)
    wrows, wrecs = batch.want_arrays()
    for p in (1, 2, 5):  # their rows: untouched
        wrows[p] = batch.rows[p] if in_place else OUT_POISON
        wrecs[p] = np.zeros(1, so.RESULT)[0]
    wrecs["skipped"][1] = 1
    wrecs["code"][[2, 5]] = -4
    assert_equal(got, (wrows, wrecs), f"in_place={in_place}")
    both = {int(s["pair"]["fix_scale"]) for s in batch.scenes}
    assert both == {0, 1} and batch.counts.max() < CAP and len({s[0] for s in batch.slots[-8:]}) == 1
    assert {int(r["rounds"]) for r in wrecs} >= {1, 2} and (wrecs["n_bad_first"] > 0).any() and (wrecs["n_bad_first"] == 0).any()


def test_the_full_batch_without_special_pairs(batch, res):
    assert_equal(res.run(), batch.want_arrays(), "full")


def test_d_sim3_rows_replace_the_records_and_skip_pairs(gpu_lib, batch, res):
    which = list(range(16, 28))
    rows = np.zeros(len(which), gpu_lib.SIM3_RESULT_DTYPE)
    rows["R12"], rows["t12"], rows["s12"], rows["has_sim3"] = batch.pairs["R12"][which], batch.pairs["t12"][which], batch.pairs["s12"][which], 1
    rows["T12"], rows["n_inliers"] = 7.0, 33  # nothing else of the record is read
    rows["has_sim3"][1] = 0
    rows["code"][2] = -3
    records = batch.pairs[which].copy()
    records["R12"], records["t12"], records["s12"] = np.nan, np.nan, -1.0  # with d_sim3 the records' Sim3 is not read
    got = res.run(which, pairs=records, sim3=rows, in_place=True)
    wrows, wrecs = batch.want_arrays(which)
    for k in (1, 2):
        wrows[k] = batch.rows[which[k]]
        wrecs[k] = np.zeros(1, so.RESULT)[0]
        wrecs["skipped"][k] = 1
    assert_equal(got, (wrows, wrecs), "d_sim3")


def test_second_call_with_fewer_pairs_and_smaller_counts(batch, res):
    """stale workspace: the call before this one compacted larger problems for more pairs"""
    res.run()
    which = [47, 33, 18]
    counts = batch.counts.copy()
    for p in which:
        a, b2 = batch.slots[p]
        counts[a], counts[b2] = counts[a] * 2 // 3, counts[b2] * 3 // 4
    try:
        res.set_counts(counts)
        got = res.run(which)
        wants = [sc.expected(batch.scenes[p], n1=counts[batch.slots[p][0]], n2=counts[batch.slots[p][1]]) for p in which]
        assert_equal(got, batch.want_arrays(which, wants), "second call")
        assert all(w[0]["n_correspondences"] < batch.want[p][0]["n_correspondences"] for w, p in zip(wants, which))
    finally:
        res.set_counts(batch.counts)
    assert_equal(res.run(which), batch.want_arrays(which), "the same pairs with the full counts again")


def test_invalid_arguments_on_the_real_handle(gpu_lib, batch, res):
    which = [0, 1]
    for field, value in (("s12", 0.0), ("th2", 0.0), ("fix_scale", 2), ("enabled", -1), ("t12", np.nan)):
        pairs = batch.pairs[which].copy()
        pairs[field][1] = value
        with pytest.raises(gpu_lib.AmosError):
            res.run(which, pairs=pairs)
    assert_equal(res.run(which), batch.want_arrays(which), "the handle works after the refusals")


def test_chain_bow_search_then_sim3_then_sim3_search_then_optimize(gpu_lib):
    """The chain of tests/test_gpu_sim3_search.py with its fourth step: amos_match_bow_kf_batch_device writes the rows of four candidate pairs,
    amos_match_sim3_batch_device reads them in place, amos_match_sim3_search_batch_device reads its d_result and rows in place, and
    amos_match_sim3_optimize_batch_device reads both again (d_sim3 = d_result, d_match12 = d_match_out = the same row): one stream, no host
    copy and no synchronisation in between, one download at the end.  Expected: the four restatements run in sequence."""
    import torch
    import kf_search_cases as kc
    import sim3_restatement as sr
    pkg = gpu_lib
    sc, _ = ss.shared()
    cap, sf = sc["capacity"], sc["sf"]
    slots = [3, 2, 4]
    rng = np.random.default_rng(9)
    sides = []
    for f in slots:
        n = int(sc["counts"][f])
        kf = ss.keyframe(sc, f)
        phys = sc["phys_of"][f, :n]
        node = np.where(phys >= 0, phys % 16, 99)
        if f != 3:
            node = np.where(rng.random(n) < 0.25, node + 100, node)
        fv = {}
        for i, nd in enumerate(node):
            fv.setdefault(int(nd), []).append(i)
        angles = np.where(phys >= 0, (phys * 37) % 360, 11.0)
        sides.append(kc.side(kf["desc"], angles, fv, (kf["points"]["flags"] & ss.lr.SKIP) == 0, np.stack([kf["kps"]["x"], kf["kps"]["y"]], 1),
                             kf["kps"]["octave"]))
    pairs_idx = [(0, 1), (1, 0), (0, 2), (2, 0)]
    rows = [kc.oracle_bow_kf(sides[a], sides[b], 0.75, 1)[1] for a, b in pairs_idx]
    d = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy()).cuda() for k, v in kc.pack(sides, cap, 1).items()}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    s3pts = np.zeros((3, cap), pkg.SIM3_POINT_DTYPE)
    mpts = np.zeros((3, cap), pkg.MAP_POINT_DTYPE)
    cell = np.full((3, cap), -1, np.int32)
    for k, f in enumerate(slots):
        n = int(sc["counts"][f])
        s3pts["flags"][k] = sr.POINT_SKIP
        s3pts["pos"][k, :n], s3pts["flags"][k, :n] = sc["points"]["pos"][f, :n], sc["points"]["flags"][f, :n] & ss.lr.SKIP
        mpts[k] = sc["points"][f]
        cell[k, :n] = ss.lr.grid_cells(sides[k]["keys"], sc["bounds"])
    cams = sc["cameras"][slots]
    sigma2 = (sf * sf).astype(f32)
    d_1, d_2 = up(np.array([p[0] for p in pairs_idx], np.int32)), up(np.array([p[1] for p in pairs_idx], np.int32))
    d_s3pts, d_mpts, d_cell = up(s3pts), up(mpts), up(cell)
    d_row = torch.full((4, cap), SEARCH_POISON, dtype=torch.int32, device="cuda")       # SearchByBoW's rows
    d_out = torch.full((4, cap), -77, dtype=torch.int32, device="cuda")              # the solver's rows, then SearchBySim3's
    d_bow_stats = torch.full((4, 4), -9, dtype=torch.int32, device="cuda")
    d_state = torch.full((4, pkg.sim3_state_bytes(cap)), 0xCD, dtype=torch.uint8, device="cuda")
    d_result = torch.full((4, 160), 0x5A, dtype=torch.uint8, device="cuda")
    d_inlier = torch.full((4, cap), 0x5A, dtype=torch.uint8, device="cuda")
    d_m1 = torch.full((4, cap), SEARCH_POISON, dtype=torch.int32, device="cuda")
    d_m2 = torch.full((4, cap), SEARCH_POISON, dtype=torch.int32, device="cuda")
    d_stats = torch.full((4, 8), -9, dtype=torch.int32, device="cuda")
    d_start = torch.zeros((3, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_items = torch.full((3, cap), -1, dtype=torch.int32, device="cuda")
    params = dict(probability=0.99, min_inliers=12, max_iterations=300)
    par = [pkg.sim3_params(500 + k, n_iterations=300, **params) for k in range(4)]
    records = np.array([pkg.sim3_search_pair(np.full(9, np.nan), [0, 0, 0], -1.0, th=7.5)] * 4)
    mt = pkg.OrbMatcher()
    torch.cuda.synchronize()
    mt.grid_build_batch_device(d_cell.data_ptr(), d["counts"].data_ptr(), 3, cap, d_start.data_ptr(), d_items.data_ptr())
    mt.bow_kf_batch_device(d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d["n_nodes"].data_ptr(), d["node_ids"].data_ptr(),
                           d["node_off"].data_ptr(), d["node_idx"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(), 4, cap, d_row.data_ptr(),
                           d_bow_stats.data_ptr(), nn_ratio=0.75, check_orientation=1, d_has_point=d["has_point"].data_ptr())
    mt.sim3_batch_device(d["kps"].data_ptr(), d["counts"].data_ptr(), d_s3pts.data_ptr(), cams, d_1.data_ptr(), d_2.data_ptr(), 4, d_row.data_ptr(), sigma2,
                         par, cap, d_state.data_ptr(), d_result.data_ptr(), d_inlier.data_ptr(), d_out.data_ptr())
    mt.sim3_search_batch_device(d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d_start.data_ptr(), d_items.data_ptr(),
                                d_mpts.data_ptr(), cams, d_1.data_ptr(), d_2.data_ptr(), records, d_out.data_ptr(), d_out.data_ptr(), d_m1.data_ptr(),
                                d_m2.data_ptr(), d_stats.data_ptr(), cap, sf, bounds=sc["bounds"], d_sim3=d_result.data_ptr())
    d_opt = torch.full((4, 256), 0x5A, dtype=torch.uint8, device="cuda")
    inv_sigma2 = (f32(1.0) / sigma2).astype(f32)
    opt_records = np.array([pkg.sim3_opt_pair(np.full(9, np.nan), [0, 0, 0], -1.0, th2=10.0, fix_scale=0)] * 4)
    mt.sim3_optimize_batch_device(d["kps"].data_ptr(), d["counts"].data_ptr(), d_s3pts.data_ptr(), cams, d_1.data_ptr(), d_2.data_ptr(), opt_records,
                                  d_out.data_ptr(), d_out.data_ptr(), d_opt.data_ptr(), cap, inv_sigma2, d_sim3=d_result.data_ptr())
    mt.sync()
    torch.cuda.synchronize()
    opt = np.frombuffer(d_opt.cpu().numpy().tobytes(), so.RESULT)
    out, m1, m2, stats = (t.cpu().numpy() for t in (d_out, d_m1, d_m2, d_stats))
    closed = gained = accepted = 0
    for k, (a, b) in enumerate(pairs_idx):
        na, nb = len(sides[a]["keys"]), len(sides[b]["keys"])
        assert np.array_equal(d_row.cpu().numpy()[k, :na], rows[k]), k
        sol = sr.Sim3Solver(sides[a]["keys"], s3pts[a, :na], cams[a], sides[b]["keys"], s3pts[b, :nb], cams[b], rows[k], sigma2, fix_scale=0, seed=500 + k)
        sol.set_ransac_parameters(**params)
        w = sol.iterate(300)
        print(f"chain pair {k}: BoW matches {(rows[k] >= 0).sum()}, has_sim3 {w.has_sim3}, inliers {w.n_inliers}, search stats {stats[k].tolist()}")
        if not w.has_sim3:
            assert (out[k] == -77).all() and (m1[k] == SEARCH_POISON).all() and stats[k].tolist() == [0, 0, 0, 0, 0, 1, 0, 0], k
            assert opt[k]["skipped"] == 1 and opt[k]["n_inliers"] == 0, k
            continue
        closed += 1
        kf1 = dict(kps=sides[a]["keys"], desc=sides[a]["desc"], points=mpts[a, :na])
        kf2 = dict(kps=sides[b]["keys"], desc=sides[b]["desc"], points=mpts[b, :nb])
        r = ss.search(kf1, kf2, cams[a], cams[b], w.R12, w.t12, w.s12, 7.5, w.match_out, sf, sc["bounds"])
        want, row = so.sim3_optimize(sides[a]["keys"], s3pts[a, :na], cams[a], sides[b]["keys"], s3pts[b, :nb], cams[b], r["match_out"], inv_sigma2,
                                     so.pair_record(w.R12, w.t12, w.s12, 10.0, 0))
        print(f"chain pair {k}: optimise: correspondences {want['n_correspondences']}, bad first {want['n_bad_first']}, inliers {want['n_inliers']}")
        assert np.array_equal(out[k, :na], row) and (out[k, na:] == -1).all(), k
        assert opt[k].tobytes() == want.tobytes(), k
        accepted += want["n_inliers"] >= 20
        assert np.array_equal(m1[k, :na], r["match1"]) and (m1[k, na:] == -1).all(), k
        assert np.array_equal(m2[k, :nb], r["match2"]) and (m2[k, nb:] == -1).all(), k
        assert np.array_equal(stats[k], ss.stats_row(r["stats"])), k
        gained += r["stats"]["n_found"] > 0
    assert closed >= 2 and gained >= 1 and accepted >= 1, "the chain's scenes are meant to close, the search to gain matches, a loop to be accepted"
    mt.close()
