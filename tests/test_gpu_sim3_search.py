"""amos_match_sim3_search_batch_device / amos_match_sim3_search on the GPU against the restatement (tests/sim3_search_restatement.py), with ==
on whole arrays: d_match_out, d_match1 (vnMatch1), d_match2 (vnMatch2) and d_stats.  tests/test_sim3_search_cpu.py holds the restatement to
the oracle and asserts that the shared scene contains every case (exits, borders, wide windows, ties, the threshold, the row's four kinds of
entry, doubled matches).  Outputs start poisoned so that "not written" is visible, and what lies behind a keyframe's count would change the
result if it were read."""
import numpy as np
import pytest

import sim3_search_restatement as ss

pytestmark = pytest.mark.gpu
f32 = np.float32
OUT_POISON = 12345


@pytest.fixture(scope="module")
def shared():
    return ss.shared()


class Resident:
    """the scene's keyframes uploaded once; every run() is one amos_match_sim3_search_batch_device call on the same handle"""

    def __init__(self, pkg, sc):
        import torch
        self.torch, self.pkg, self.sc = torch, pkg, sc
        self.cap, self.nf = sc["capacity"], len(sc["counts"])
        kps, desc, points = sc["kps"].copy(), sc["desc"].copy(), sc["points"].copy()
        self.cell = np.full((self.nf, self.cap), 7 * 48 + 3, np.int32)
        for f, n in enumerate(sc["counts"]):  # poison that WOULD take part if an index past a count were read
            kps["x"][f, n:], kps["y"][f, n:], kps["octave"][f, n:] = 100.0, 100.0, 1
            desc[f, n:] = 0xFF
            points["flags"][f, n:], points["pos"][f, n:], points["max_distance"][f, n:] = 0, (0.0, 0.0, 3.0), 4.0
            self.cell[f, :n] = ss.lr.grid_cells(kps[f, :n], sc["bounds"])
        self.d_kps, self.d_desc, self.d_points, self.d_cell = self.up(kps), self.up(desc), self.up(points), self.up(self.cell)
        self.d_start = torch.zeros((self.nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
        self.d_items = torch.full((self.nf, self.cap), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.mt = pkg.OrbMatcher()
        self.set_counts(sc["counts"])

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def set_counts(self, counts):
        self.d_counts = self.up(np.asarray(counts, np.int32))
        self.mt.grid_build_batch_device(self.d_cell.data_ptr(), self.d_counts.data_ptr(), self.nf, self.cap, self.d_start.data_ptr(), self.d_items.data_ptr())
        self.mt.sync()

    def run(self, which=None, pairs=None, sim3=None, in_place=False, slots1=None, slots2=None, rows=None, cameras=None):
        """one batch call over the pairs `which` of the scene -> (match_out, match1, match2 [pairs][cap], stats [pairs][8])"""
        torch, sc, cap = self.torch, self.sc, self.cap
        which = list(range(len(sc["pairs"]))) if which is None else list(which)
        n = len(which)
        pairs = sc["pairs"][which] if pairs is None else pairs
        s1 = sc["slots1"][which] if slots1 is None else slots1
        s2 = sc["slots2"][which] if slots2 is None else slots2
        d_rows = self.up(sc["rows"][which] if rows is None else rows)
        d_out = d_rows if in_place else torch.full((n, cap), OUT_POISON, dtype=torch.int32, device="cuda")
        d_m1 = torch.full((n, cap), OUT_POISON, dtype=torch.int32, device="cuda")
        d_m2 = torch.full((n, cap), OUT_POISON, dtype=torch.int32, device="cuda")
        d_stats = torch.full((n, 8), -9, dtype=torch.int32, device="cuda")
        d_s1, d_s2 = self.up(np.asarray(s1, np.int32)), self.up(np.asarray(s2, np.int32))
        d_sim3 = None if sim3 is None else self.up(sim3)
        torch.cuda.synchronize()
        self.mt.sim3_search_batch_device(self.d_kps.data_ptr(), self.d_desc.data_ptr(), self.d_counts.data_ptr(), self.d_start.data_ptr(),
                                         self.d_items.data_ptr(), self.d_points.data_ptr(), sc["cameras"] if cameras is None else cameras, d_s1.data_ptr(), d_s2.data_ptr(), pairs,
                                         d_rows.data_ptr(), d_out.data_ptr(), d_m1.data_ptr(), d_m2.data_ptr(), d_stats.data_ptr(), cap, sc["sf"],
                                         bounds=sc["bounds"], d_sim3=None if d_sim3 is None else d_sim3.data_ptr())
        self.mt.sync()
        torch.cuda.synchronize()
        view = lambda t: np.frombuffer(t.cpu().numpy().tobytes(), np.int32).reshape(n, -1)
        return view(d_out), view(d_m1), view(d_m2), view(d_stats)


@pytest.fixture(scope="module")
def res(gpu_lib, shared):
    return Resident(gpu_lib, shared[0])


def sim3_rows(pkg, pairs):
    """the solver's result records holding the pairs' Sim3"""
    r = np.zeros(len(pairs), pkg.SIM3_RESULT_DTYPE)
    r["R12"], r["t12"], r["s12"], r["has_sim3"] = pairs["R12"], pairs["t12"], pairs["s12"], 1
    r["T12"], r["n_inliers"] = 7.0, 33  # nothing else of the record is read
    return r


def assert_equal(got, want, what):
    for name, g, w in zip(("match_out", "match1", "match2", "stats"), got, want):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())


@pytest.mark.parametrize("source", ["host_records", "d_sim3"])
def test_batch_equals_the_restatement(gpu_lib, shared, res, source):
    sc, results = shared
    want = ss.expected_arrays(sc, results)
    if source == "host_records":
        got = res.run()
    else:
        records = sc["pairs"].copy()
        records["R12"], records["t12"], records["s12"] = np.nan, np.nan, -1.0  # with d_sim3 the records' Sim3 is not read
        got = res.run(pairs=records, sim3=sim3_rows(gpu_lib, sc["pairs"]))
    for p, name in enumerate(sc["names"]):
        print(name, got[3][p].tolist())
    assert_equal(got, want, source)


def test_in_place_equals_out_of_place(shared, res):
    sc, results = shared
    assert_equal(res.run(in_place=True), ss.expected_arrays(sc, results), "in place")


def test_skipped_pairs_keep_their_rows(gpu_lib, shared, res):
    sc, results = shared
    # host records: pair 0 disabled, pair 5 with keyframe 1's slot outside the frames, pair 7 with keyframe 2's
    records = sc["pairs"].copy()
    records["enabled"][0] = 0
    records["th"][0] = -1.0  # (a disabled pair's record is not looked into)
    s1, s2 = sc["slots1"].copy(), sc["slots2"].copy()
    s1[5], s2[7] = len(sc["counts"]), -1
    want = list(ss.expected_arrays(sc, results))
    for a in want[:3]:
        a[[0, 5, 7]] = OUT_POISON
    want[3][[0, 5, 7]] = 0
    want[3][0, ss.STATS.index("skipped")] = 1
    want[3][[5, 7], ss.STATS.index("code")] = -4
    assert_equal(res.run(pairs=records, slots1=s1, slots2=s2), want, "enabled = 0 and slots outside the frames")
    # d_sim3: pair 1 without a Sim3, pair 2 refused by the solver; in place, so their rows stay the input's
    rows = sim3_rows(gpu_lib, sc["pairs"])
    rows["has_sim3"][1] = 0
    rows["code"][2] = -3
    want = list(ss.expected_arrays(sc, results))
    want[0][[1, 2]] = sc["rows"][[1, 2]]
    want[1][[1, 2]] = want[2][[1, 2]] = OUT_POISON
    want[3][[1, 2]] = 0
    want[3][[1, 2], ss.STATS.index("skipped")] = 1
    assert_equal(res.run(sim3=rows, in_place=True), want, "has_sim3 = 0 and code != 0")


def test_second_call_with_fewer_pairs_and_smaller_counts(shared, res):
    """stale scratch: the call before this one marked vbAlreadyMatched2 for eleven pairs of larger keyframes"""
    sc, results = shared
    res.run()
    counts = sc["counts"].copy()
    counts[3], counts[2] = 500, 257
    which = [0, 2, 5]
    try:
        res.set_counts(counts)
        got = res.run(which)
        sub = [ss.run_pair(sc, p, counts=counts) for p in which]
        want = ss.expected_arrays(dict(sc, rows=sc["rows"][which]), sub)
        assert_equal(got, want, "second call")
        assert any((sc["rows"][p][:counts[sc["slots1"][p]]] >= counts[sc["slots2"][p]]).sum() > 3 for p in which)  # entries that now lie past N2
    finally:
        res.set_counts(sc["counts"])
    assert_equal(res.run(), ss.expected_arrays(sc, results), "the full call again")


def test_host_form_equals_the_restatement(gpu_lib, shared):
    sc, results = shared
    mt = gpu_lib.OrbMatcher()
    for name in ("truth", "empty_1", "empty_2", "double", "same"):
        p = sc["names"].index(name)
        a, b = int(sc["slots1"][p]), int(sc["slots2"][p])
        k1, k2 = ss.keyframe(sc, a), ss.keyframe(sc, b)
        n1 = len(k1["kps"])
        out, m1, m2, stats = mt.sim3_search(dict(keys_un=k1["kps"], desc=k1["desc"]), k1["points"], dict(keys_un=k2["kps"], desc=k2["desc"]), k2["points"],
                                            sc["cameras"][[a, b]], sc["pairs"][p], sc["sf"], sc["rows"][p][:n1], bounds=sc["bounds"])
        w = results[p]
        assert np.array_equal(out, w["match_out"]) and np.array_equal(m1, w["match1"]) and np.array_equal(m2, w["match2"]), name
        assert np.array_equal(np.array(stats.tolist(), np.int32), ss.stats_row(w["stats"])), name
    # a disabled pair: the stats record alone
    p = sc["names"].index("truth")
    a, b = int(sc["slots1"][p]), int(sc["slots2"][p])
    k1, k2 = ss.keyframe(sc, a), ss.keyframe(sc, b)
    off = sc["pairs"][p].copy()
    off["enabled"] = 0
    row = sc["rows"][p][:len(k1["kps"])]
    out, m1, m2, stats = mt.sim3_search(dict(keys_un=k1["kps"], desc=k1["desc"]), k1["points"], dict(keys_un=k2["kps"], desc=k2["desc"]), k2["points"],
                                        sc["cameras"][[a, b]], off, sc["sf"], row, bounds=sc["bounds"])
    assert np.array_equal(out, row) and (m1 == -1).all() and (m2 == -1).all() and stats["skipped"] == 1 and stats["n_found"] == 0
    mt.close()


def test_invalid_arguments_on_the_real_handle(gpu_lib, shared, res):
    sc, results = shared
    bad_cams = sc["cameras"].copy()
    bad_cams["fx"][1] = np.inf
    for over in (dict(pairs=np.array([gpu_lib.sim3_search_pair(np.eye(3), [0, 0, 0], 0.0)] * 11)),
                 dict(pairs=np.array([gpu_lib.sim3_search_pair(np.eye(3), [0, 0, 0], 1.0, th=0.0)] * 11)), dict(cameras=bad_cams)):
        with pytest.raises(gpu_lib.AmosError):
            res.run(**over)
    assert_equal(res.run(), ss.expected_arrays(sc, results), "the handle works after the refusals")


def test_chain_bow_search_then_sim3_then_sim3_search_on_resident_arrays(gpu_lib, shared):
    """amos_match_bow_kf_batch_device writes the rows of four candidate pairs, amos_match_sim3_batch_device (find: up to 300 iterations) reads
    them in place and leaves d_result and d_match_out, amos_match_sim3_search_batch_device reads both in place (d_sim3 = d_result, d_match12 =
    d_match_out = the solver's row): one stream, no host copy and no synchronisation in between.  The keyframes are three of the shared
    scene's, whose map points obey one similarity per pair; a quarter of keyframe 2's and 4's features sit in another vocabulary node than
    their partners, so SearchByBoW misses them and SearchBySim3 has matches to gain.  Expected: the oracle's rows through
    tests/sim3_restatement.py through tests/sim3_search_restatement.py."""
    import torch
    import kf_search_cases as kc
    import sim3_restatement as sr
    pkg = gpu_lib
    sc, _ = shared
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
    d_row = torch.full((4, cap), OUT_POISON, dtype=torch.int32, device="cuda")       # SearchByBoW's rows
    d_out = torch.full((4, cap), -77, dtype=torch.int32, device="cuda")              # the solver's rows, then SearchBySim3's
    d_bow_stats = torch.full((4, 4), -9, dtype=torch.int32, device="cuda")
    d_state = torch.full((4, pkg.sim3_state_bytes(cap)), 0xCD, dtype=torch.uint8, device="cuda")
    d_result = torch.full((4, 160), 0x5A, dtype=torch.uint8, device="cuda")
    d_inlier = torch.full((4, cap), 0x5A, dtype=torch.uint8, device="cuda")
    d_m1 = torch.full((4, cap), OUT_POISON, dtype=torch.int32, device="cuda")
    d_m2 = torch.full((4, cap), OUT_POISON, dtype=torch.int32, device="cuda")
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
    mt.sync()
    torch.cuda.synchronize()
    out, m1, m2, stats = (t.cpu().numpy() for t in (d_out, d_m1, d_m2, d_stats))
    closed = gained = 0
    for k, (a, b) in enumerate(pairs_idx):
        na, nb = len(sides[a]["keys"]), len(sides[b]["keys"])
        assert np.array_equal(d_row.cpu().numpy()[k, :na], rows[k]), k
        sol = sr.Sim3Solver(sides[a]["keys"], s3pts[a, :na], cams[a], sides[b]["keys"], s3pts[b, :nb], cams[b], rows[k], sigma2, fix_scale=0, seed=500 + k)
        sol.set_ransac_parameters(**params)
        w = sol.iterate(300)
        print(f"chain pair {k}: BoW matches {(rows[k] >= 0).sum()}, has_sim3 {w.has_sim3}, inliers {w.n_inliers}, search stats {stats[k].tolist()}")
        if not w.has_sim3:
            assert (out[k] == -77).all() and (m1[k] == OUT_POISON).all() and stats[k].tolist() == [0, 0, 0, 0, 0, 1, 0, 0], k
            continue
        closed += 1
        kf1 = dict(kps=sides[a]["keys"], desc=sides[a]["desc"], points=mpts[a, :na])
        kf2 = dict(kps=sides[b]["keys"], desc=sides[b]["desc"], points=mpts[b, :nb])
        r = ss.search(kf1, kf2, cams[a], cams[b], w.R12, w.t12, w.s12, 7.5, w.match_out, sf, sc["bounds"])
        assert np.array_equal(out[k, :na], r["match_out"]) and (out[k, na:] == -1).all(), k
        assert np.array_equal(m1[k, :na], r["match1"]) and (m1[k, na:] == -1).all(), k
        assert np.array_equal(m2[k, :nb], r["match2"]) and (m2[k, nb:] == -1).all(), k
        assert np.array_equal(stats[k], ss.stats_row(r["stats"])), k
        gained += r["stats"]["n_found"] > 0
    assert closed >= 2 and gained >= 1, "the chain's scenes are meant to close, and the search to gain matches"
    mt.close()
