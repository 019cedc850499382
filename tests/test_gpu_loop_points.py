"""amos_match_loop_points_batch_device on the GPU against the plain-Python restatement (tests/loop_points_restatement.py): whole arrays with ==
-- every d_loop_match row with its padding, every stats record, and the entry rows, which the call must not write -- on the scene
tests/test_loop_points_cpu.py shows to hold every case; the d_opt form and its skips; both sources of spAlreadyFound; eight queries in one
call; empty lists and keyframes; a reused handle; the hand-made greedy case; and the resident chain BoW search -> Sim3Solver -> SearchBySim3
-> OptimizeSim3 -> this search on one stream."""
import numpy as np
import pytest

import local_points_restatement as lr  # grid_cells
import loop_points_restatement as lp

pytestmark = pytest.mark.gpu

POISON = -77   # what d_loop_match and d_stats hold on entry
ROW_PAD = 7    # the padding of an entry row: occupied, and beyond the keyframe's features (it counts for nothing)
f32 = np.float32


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Resident:
    """keyframes [(kps, desc)] uploaded once into [frames][cap] arrays with their grids, and a matcher handle"""

    def __init__(self, pkg, kfs, bounds, cap):
        import torch
        self.pkg, self.kfs, self.bounds, self.cap, self.nf = pkg, kfs, bounds, cap, len(kfs)
        kps, desc = np.zeros((self.nf, cap), pkg.KP_DTYPE), np.zeros((self.nf, cap, 32), np.uint8)
        cell, counts = np.full((self.nf, cap), -1, np.int32), np.zeros(self.nf, np.int32)
        for f, (k, d) in enumerate(kfs):
            n = len(k)
            counts[f] = n
            kps[f, :n], desc[f, :n], cell[f, :n] = k, d, lr.grid_cells(k, bounds)
        self.d_kps, self.d_desc, self.d_counts, d_cell = up(kps), up(desc), up(counts), up(cell)
        self.d_start = torch.zeros((self.nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
        self.d_items = torch.full((self.nf, cap), -1, dtype=torch.int32, device="cuda")
        self.mt = pkg.OrbMatcher()
        self.mt.grid_build_batch_device(d_cell.data_ptr(), self.d_counts.data_ptr(), self.nf, cap, self.d_start.data_ptr(), self.d_items.data_ptr())
        self.mt.sync()

    def run(self, points, first, count, queries, rows, sf, maps=None, found=None, opt=None):
        """one call -> (loop_match [queries][cap], stats, the entry rows as they stand behind the call, as they were uploaded)"""
        import torch
        pkg, cap, nq = self.pkg, self.cap, len(queries)
        row = np.full((nq, cap), ROW_PAD, np.int32)
        pf2 = np.full((nq, cap), -1, np.int32)
        for k in range(nq):
            row[k, :len(rows[k])] = rows[k]
            if maps is not None and maps[k] is not None:
                pf2[k, :len(maps[k])] = maps[k]
        pts = np.ascontiguousarray(points, pkg.MAP_POINT_DTYPE) if len(points) else np.zeros(1, pkg.MAP_POINT_DTYPE)
        d_pts, d_row, d_pf2 = up(pts), up(row), up(pf2)
        d_found = None if found is None else up(np.ascontiguousarray(found, np.uint8) if len(found) else np.zeros(1, np.uint8))
        d_opt = None if opt is None else up(np.ascontiguousarray(opt, pkg.SIM3_OPT_RESULT_DTYPE))
        d_loop = torch.full((nq, cap), POISON, dtype=torch.int32, device="cuda")
        d_stats = torch.full((nq, 8), POISON, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.mt.loop_points_batch_device(self.d_kps.data_ptr(), self.d_desc.data_ptr(), self.d_counts.data_ptr(), self.d_start.data_ptr(),
                                         self.d_items.data_ptr(), self.nf, d_pts.data_ptr(), len(points), first, count, queries, d_row.data_ptr(),
                                         d_loop.data_ptr(), d_stats.data_ptr(), cap, sf, bounds=self.bounds,
                                         d_opt=None if d_opt is None else d_opt.data_ptr(), d_found=None if d_found is None else d_found.data_ptr(),
                                         d_point_of_feature2=None if maps is None else d_pf2.data_ptr())
        self.mt.sync()
        torch.cuda.synchronize()
        return (d_loop.cpu().numpy(), np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.LOOP_POINTS_STATS_DTYPE),
                np.frombuffer(d_row.cpu().numpy().tobytes(), np.int32).reshape(nq, cap), row)

    def close(self):
        self.mt.close()


def restate(kfs, points, first, count, queries, rows, sf, bounds, maps=None, found=None, opt=None):
    out = []
    for k, q in enumerate(queries):
        kps, desc = kfs[int(q["frame"])]
        a, c = int(first[k]), int(count[k])
        o = None if opt is None else dict(skipped=int(opt["skipped"][k]), code=int(opt["code"][k]), n_inliers=int(opt["n_inliers"][k]), Scw=opt["Scw"][k])
        out.append(lp.search(kps, desc, points[a:a + c], q, rows[k], None if found is None else found[a:a + c], None if maps is None else maps[k],
                             sf, bounds, opt=o))
    return out


def assert_call(got, want, kfs, queries):
    """every query of one device call equals its restatement: whole arrays"""
    loop, stats, row_after, row_before = got
    assert np.array_equal(row_after, row_before), "the entry rows are not written"
    for k, (q, w) in enumerate(zip(queries, want)):
        n = len(kfs[int(q["frame"])][0])
        print(f"query {k}:", {name: (int(stats[name][k]), int(w[name])) for name in lp.STATS})
        assert tuple(int(stats[name][k]) for name in lp.STATS) == tuple(int(w[name]) for name in lp.STATS), k
        if w["skipped"]:  # nothing but the stats record is written
            assert (loop[k] == POISON).all(), k
            continue
        assert np.array_equal(loop[k, :n], w["loop_match"]), k
        assert (loop[k, n:] == -1).all(), k


@pytest.fixture(scope="module")
def shared():
    return lp.shared()


@pytest.fixture(scope="module")
def resident(gpu_lib, shared):
    sc, _ = shared
    r = Resident(gpu_lib, sc["kfs"], sc["bounds"], sc["capacity"])
    yield r
    r.close()


def scene_args(sc):
    return dict(points=sc["points"], first=sc["first"], count=sc["count"], queries=sc["queries"], rows=sc["rows"], sf=sc["sf"])


def test_shared_scene_with_host_scw(resident, shared):
    sc, want = shared
    got = resident.run(maps=sc["maps"], found=sc["found"], **scene_args(sc))
    assert_call(got, want, sc["kfs"], sc["queries"])
    assert got[1]["accepted"].tolist() == [1, 0] and got[1]["n_researched"][0] >= 3 and got[1]["n_total"][0] >= 40 > got[1]["n_total"][1] > 0


def test_d_opt_rows_supply_scw_and_skip_queries(gpu_lib, resident, shared):
    """Six queries on the scene's first: rows that skip by `skipped`, by `code` and by n_inliers = 19, one at 20 that runs, one with another
    Scw, and one disabled on the host.  The records' own Scw is not finite: it must not be read."""
    sc, want = shared
    q0 = sc["queries"][0]
    queries = np.array([q0] * 6, lp.QUERY)
    queries["Scw"] = np.nan
    queries["enabled"][5] = 0
    opt = np.zeros(6, gpu_lib.SIM3_OPT_RESULT_DTYPE)
    opt["Scw"], opt["n_inliers"] = q0["Scw"], 30
    opt["skipped"][0], opt["code"][1], opt["n_inliers"][2], opt["n_inliers"][3] = 1, -4, 19, 20
    opt["Scw"][4] = lp.scw_of(0.93, 0.03, -0.02, 0.005, [0.05, -0.05, 0.1]).reshape(16)
    first, count = np.zeros(6, np.int32), np.full(6, sc["count"][0], np.int32)
    rows, maps = [sc["rows"][0]] * 6, [sc["maps"][0]] * 6
    args = dict(points=sc["points"], first=first, count=count, queries=queries, rows=rows, sf=sc["sf"], maps=maps, found=sc["found"], opt=opt)
    got = resident.run(**args)
    args.pop("sf")
    w = restate(sc["kfs"], sf=sc["sf"], bounds=sc["bounds"], **args)
    assert_call(got, w, sc["kfs"], queries)
    assert [int(x["skipped"]) for x in w] == [1, 1, 1, 0, 0, 1]
    assert np.array_equal(w[3]["loop_match"], want[0]["loop_match"]) and not np.array_equal(w[4]["loop_match"], want[0]["loop_match"])


@pytest.mark.parametrize("source", ["bytes", "map", "both"])
def test_the_sources_of_already_found(resident, shared, source):
    sc, want = shared
    queries = sc["queries"].copy()
    queries["found_from_match"] = 0 if source == "bytes" else 1
    args = scene_args(sc)
    args.update(queries=queries, maps=None if source == "bytes" else sc["maps"], found=None if source == "map" else sc["found"])
    got = resident.run(**args)
    args.pop("sf")
    w = restate(sc["kfs"], sf=sc["sf"], bounds=sc["bounds"], **args)
    assert_call(got, w, sc["kfs"], queries)
    if source != "both":  # each source alone finds fewer points than both
        assert w[0]["n_candidates"] > want[0]["n_candidates"]


def test_eight_queries_with_their_own_ranges(resident, shared):
    """Eight queries in one call over both keyframes: different ranges of the two lists, queries 2 and 5 sharing one range under different
    rows, one with th = 4 and one with max_dist = 30."""
    sc, _ = shared
    a, b = int(sc["count"][0]), int(sc["count"][1])
    ranges = [(0, a), (a, b), (100, 257), (0, 64), (65, 130), (100, 257), (a + 5, 31), (300, 300)]
    frames = [0, 1, 0, 0, 0, 0, 1, 0]
    queries = np.array([sc["queries"][f] for f in frames], lp.QUERY)
    queries["found_from_match"] = 0
    queries["th"][3], queries["max_dist"][4], queries["min_total"][7] = 4.0, 30, 500
    rng = np.random.default_rng(21)
    rows = [sc["rows"][f].copy() for f in frames]
    rows[5] = np.where(rng.random(len(rows[5])) < 0.3, 3, -1).astype(np.int32)
    first, count = np.array([r[0] for r in ranges], np.int32), np.array([r[1] for r in ranges], np.int32)
    args = dict(points=sc["points"], first=first, count=count, queries=queries, rows=rows, found=sc["found"])
    got = resident.run(sf=sc["sf"], **args)
    w = restate(sc["kfs"], sf=sc["sf"], bounds=sc["bounds"], **args)
    assert_call(got, w, sc["kfs"], queries)
    assert not np.array_equal(w[2]["loop_match"], w[5]["loop_match"]) and w[7]["accepted"] == 0 and w[0]["accepted"] == 1
    assert all(x["n_matches"] > 0 for x in w)


def test_no_points_no_features_capacity_above_the_counts_and_a_reused_handle(gpu_lib, shared):
    """A keyframe without features beside the scene's, a query without points, capacity 512 above every count; then on the same handle a
    second call with fewer queries, fewer points and the same answers."""
    sc, want = shared
    k0, d0 = sc["kfs"][0]
    kfs = [sc["kfs"][0], (k0[:0], d0[:0]), sc["kfs"][1]]
    r = Resident(gpu_lib, kfs, sc["bounds"], 512)
    queries = np.array([sc["queries"][0], sc["queries"][0], sc["queries"][0], sc["queries"][1]], lp.QUERY)
    queries["frame"] = [0, 1, 0, 2]
    first, count = np.array([0, 0, 17, sc["first"][1]], np.int32), np.array([sc["count"][0], sc["count"][0], 0, sc["count"][1]], np.int32)
    rows = [sc["rows"][0], np.zeros(0, np.int32), sc["rows"][0], sc["rows"][1]]
    maps = [sc["maps"][0], sc["maps"][0], sc["maps"][0], sc["maps"][1]]
    args = dict(points=sc["points"], first=first, count=count, queries=queries, rows=rows, maps=maps, found=sc["found"])
    got = r.run(sf=sc["sf"], **args)
    w = restate(kfs, sf=sc["sf"], bounds=sc["bounds"], **args)
    assert_call(got, w, kfs, queries)
    assert np.array_equal(w[0]["loop_match"], want[0]["loop_match"]) and np.array_equal(w[3]["loop_match"], want[1]["loop_match"])
    assert w[1]["n_in_view"] > 100 and w[1]["n_matches"] == 0 and w[1]["n_total"] == 0
    assert w[2]["n_candidates"] == 0 and w[2]["n_total"] == int((sc["rows"][0] != -1).sum())
    small = dict(points=sc["points"][:200], first=first[:1], count=np.array([130], np.int32), queries=queries[:1], rows=rows[:1], maps=maps[:1],
                 found=sc["found"][:200])
    got2 = r.run(sf=sc["sf"], **small)
    assert_call(got2, restate(kfs, sf=sc["sf"], bounds=sc["bounds"], **small), kfs, queries[:1])
    again = r.run(sf=sc["sf"], **args)
    assert np.array_equal(again[0], got[0]) and again[1].tobytes() == got[1].tobytes()
    r.close()


def test_greedy_order_by_hand(gpu_lib):
    """Three points whose windows hold the same two features: the first takes A, the second finds A taken and takes B, the third finds both
    taken and gets nothing; alone it takes B."""
    h = lp.hand_greedy()
    kfs = [(h["kps"], h["desc"])]
    r = Resident(gpu_lib, kfs, lp.BOUNDS, 2)
    queries = np.array([h["query"]], lp.QUERY)
    free = [np.full(2, -1, np.int32)]
    for pts, expected, researched in ((h["points"], h["expected"], 1), (h["points"][2:], np.array([-1, 0], np.int32), 0),
                                      (h["points"][::-1], np.array([1, 0], np.int32), 1)):
        args = dict(points=pts, first=np.zeros(1, np.int32), count=np.array([len(pts)], np.int32), queries=queries, rows=free)
        got = r.run(sf=lp.SCALE, **args)
        w = restate(kfs, sf=lp.SCALE, bounds=lp.BOUNDS, **args)
        assert_call(got, w, kfs, queries)
        assert np.array_equal(got[0][0], expected) and got[1]["n_researched"][0] == researched
    r.close()


def test_chain_bow_search_sim3_sim3_search_optimize_loop_points(gpu_lib):
    """The chain of tests/test_gpu_sim3_optimization.py with its fifth step: amos_match_loop_points_batch_device reads OptimizeSim3's result
    records (d_opt: the Scw and the nInliers >= 20 test) and the row it left in d_match_out in place (d_matched, with found_from_match through
    the identity map: keyframe 2's point at feature j is point j of the query's list).  One stream, no host copy and no synchronisation in
    between, one download at the end.  Expected: the five restatements run in sequence."""
    import torch
    import kf_search_cases as kc
    import sim3_optimization_restatement as so
    import sim3_restatement as sr
    import sim3_search_restatement as ss
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
    d = {k: up(v) for k, v in kc.pack(sides, cap, 1).items()}
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
    inv_sigma2 = (f32(1.0) / sigma2).astype(f32)
    d_1, d_2 = up(np.array([p[0] for p in pairs_idx], np.int32)), up(np.array([p[1] for p in pairs_idx], np.int32))
    d_s3pts, d_mpts, d_cell = up(s3pts), up(mpts), up(cell)
    d_row = torch.full((4, cap), 12345, dtype=torch.int32, device="cuda")
    d_out = torch.full((4, cap), -77, dtype=torch.int32, device="cuda")
    d_bow_stats = torch.full((4, 4), -9, dtype=torch.int32, device="cuda")
    d_state = torch.full((4, pkg.sim3_state_bytes(cap)), 0xCD, dtype=torch.uint8, device="cuda")
    d_result = torch.full((4, 160), 0x5A, dtype=torch.uint8, device="cuda")
    d_inlier = torch.full((4, cap), 0x5A, dtype=torch.uint8, device="cuda")
    d_m1 = torch.full((4, cap), 12345, dtype=torch.int32, device="cuda")
    d_m2 = torch.full((4, cap), 12345, dtype=torch.int32, device="cuda")
    d_stats = torch.full((4, 8), -9, dtype=torch.int32, device="cuda")
    d_opt = torch.full((4, 256), 0x5A, dtype=torch.uint8, device="cuda")
    d_start = torch.zeros((3, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_items = torch.full((3, cap), -1, dtype=torch.int32, device="cuda")
    d_loop = torch.full((4, cap), POISON, dtype=torch.int32, device="cuda")
    d_loop_stats = torch.full((4, 8), POISON, dtype=torch.int32, device="cuda")
    d_pf2 = up(np.tile(np.arange(cap, dtype=np.int32), (4, 1)))
    params = dict(probability=0.99, min_inliers=12, max_iterations=300)
    par = [pkg.sim3_params(500 + k, n_iterations=300, **params) for k in range(4)]
    records = np.array([pkg.sim3_search_pair(np.full(9, np.nan), [0, 0, 0], -1.0, th=7.5)] * 4)
    opt_records = np.array([pkg.sim3_opt_pair(np.full(9, np.nan), [0, 0, 0], -1.0, th2=10.0, fix_scale=0)] * 4)
    counts = [len(s["keys"]) for s in sides]
    queries = np.array([lp.query(a, np.full(16, np.nan), intr=tuple(float(cams[a][k]) for k in ("fx", "fy", "cx", "cy")), found_from_match=1)
                        for a, _ in pairs_idx], lp.QUERY)
    first, count = np.array([b * cap for _, b in pairs_idx], np.int32), np.array([counts[b] for _, b in pairs_idx], np.int32)
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
    mt.sim3_optimize_batch_device(d["kps"].data_ptr(), d["counts"].data_ptr(), d_s3pts.data_ptr(), cams, d_1.data_ptr(), d_2.data_ptr(), opt_records,
                                  d_out.data_ptr(), d_out.data_ptr(), d_opt.data_ptr(), cap, inv_sigma2, d_sim3=d_result.data_ptr())
    mt.loop_points_batch_device(d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d_start.data_ptr(), d_items.data_ptr(), 3,
                                d_mpts.data_ptr(), 3 * cap, first, count, queries, d_out.data_ptr(), d_loop.data_ptr(), d_loop_stats.data_ptr(), cap, sf,
                                bounds=sc["bounds"], d_opt=d_opt.data_ptr(), d_point_of_feature2=d_pf2.data_ptr())
    mt.sync()
    torch.cuda.synchronize()
    opt = np.frombuffer(d_opt.cpu().numpy().tobytes(), so.RESULT)
    out, loop = d_out.cpu().numpy(), d_loop.cpu().numpy()
    stats = np.frombuffer(d_loop_stats.cpu().numpy().tobytes(), pkg.LOOP_POINTS_STATS_DTYPE)
    mt.close()
    ran = gained = 0
    for k, (a, b) in enumerate(pairs_idx):
        na, nb = counts[a], counts[b]
        sol = sr.Sim3Solver(sides[a]["keys"], s3pts[a, :na], cams[a], sides[b]["keys"], s3pts[b, :nb], cams[b], rows[k], sigma2, fix_scale=0, seed=500 + k)
        sol.set_ransac_parameters(**params)
        w = sol.iterate(300)
        if not w.has_sim3:
            assert opt[k]["skipped"] == 1 and stats[k]["skipped"] == 1 and (loop[k] == POISON).all(), k
            continue
        kf1 = dict(kps=sides[a]["keys"], desc=sides[a]["desc"], points=mpts[a, :na])
        kf2 = dict(kps=sides[b]["keys"], desc=sides[b]["desc"], points=mpts[b, :nb])
        r = ss.search(kf1, kf2, cams[a], cams[b], w.R12, w.t12, w.s12, 7.5, w.match_out, sf, sc["bounds"])
        res, row = so.sim3_optimize(sides[a]["keys"], s3pts[a, :na], cams[a], sides[b]["keys"], s3pts[b, :nb], cams[b], r["match_out"], inv_sigma2,
                                    so.pair_record(w.R12, w.t12, w.s12, 10.0, 0))
        assert opt[k].tobytes() == res.tobytes() and np.array_equal(out[k, :na], row), k
        o = dict(skipped=int(res["skipped"]), code=int(res["code"]), n_inliers=int(res["n_inliers"]), Scw=res["Scw"])
        want = lp.search(sides[a]["keys"], sides[a]["desc"], mpts[b, :nb], queries[k], row, None, np.arange(cap, dtype=np.int32), sf, sc["bounds"], opt=o)
        print(f"chain pair {k}: optimiser inliers {res['n_inliers']}:", {name: (int(stats[name][k]), int(want[name])) for name in lp.STATS})
        assert tuple(int(stats[name][k]) for name in lp.STATS) == tuple(int(want[name]) for name in lp.STATS), k
        if want["skipped"]:
            assert (loop[k] == POISON).all(), k
            continue
        ran += 1
        gained += want["n_matches"] > 0
        assert np.array_equal(loop[k, :na], want["loop_match"]) and (loop[k, na:] == -1).all(), k
        assert want["n_total"] == int((row != -1).sum()) + want["n_matches"]
    assert ran >= 1 and gained >= 1, "a candidate is meant to pass the optimiser's inlier test and the search to gain matches"
