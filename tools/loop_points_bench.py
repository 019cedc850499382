#!/usr/bin/env python3
"""Times ComputeSim3's SearchByProjection(pKF, Scw, vpPoints, vpMatched, 10) (ORBmatcher.cc:388-512) on synthetic keyframes of 500, 1 000 and
2 000 features at 640 x 480 against loop lists of 1 000, 4 000 and 10 000 points (several points per feature: shared windows), an eighth
of the features occupied on entry:
  - the resident path (amos_match_loop_points_batch_device: the launches of one call) between two HIP events on the matcher's stream, one
    query per call and 8 queries per call (eight candidates' lists against one keyframe), medians of 30 calls after warm-up;
  - the host form (amos_match_loop_points through OrbMatcher.loop_points) and the C++ drop-in ORB_SLAM2::SearchByProjection over it
    (std::chrono inside the harness around the call, gathers and write-back included), wall clock, medians of 30;
  - the existing host class's search alone on the same scene (amos_host_search_by_projection_sim of tests/host: the view-level search of
    ORBmatcher.h, one amos_match_list_distances call and a host loop; its pre-filter is computed outside the timed call), wall clock,
    median of 30.
Prints one JSON line per size (milliseconds)."""
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

QUERIES = 8
SIZES = ((500, 1000), (1000, 4000), (2000, 10000))  # features of the keyframe, loop points


def wall(fn, reps=30):
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms[1:]))


def bench_scene(lp, n, m, seed):
    """a keyframe of n features and a loop list of m points made from them -> (kps, desc, points, Scw, entry row)"""
    rng = np.random.default_rng(seed)
    kps = np.zeros(n, lp.lr.hb.KP)
    kps["x"] = rng.uniform(lp.BOUNDS[0] + 1, lp.BOUNDS[1] - 1, n)
    kps["y"] = rng.uniform(lp.BOUNDS[2] + 1, lp.BOUNDS[3] - 1, n)
    kps["octave"], kps["size"] = rng.integers(0, len(lp.SCALE), n), 31
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    S = lp.scw_of(0.93, 0.01, -0.02, 0.005, [0.05, -0.02, 0.1])
    points, _ = lp.make_points(rng, (kps, desc), m, S)
    row = np.where(rng.random(n) < 0.125, lp.MATCHED_ELSEWHERE, -1).astype(np.int32)
    return kps, desc, points, S, row


def main(reps=30):
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import adaptor_prefilter as ap
    import host_binding as hb
    import host_loop_points_binding as hlb
    import loop_points_restatement as lp
    side = torch.cuda.Stream()  # the matcher issues on it, the events are recorded on it
    torch.cuda.set_stream(side)
    mt = pkg.OrbMatcher(stream=side.cuda_stream)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def events(call):
        times = []
        for rep in range(reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if rep >= 5:
                times.append(e0.elapsed_time(e1))
        mt.sync()
        return round(float(np.median(times)), 4)

    sf, bounds = lp.SCALE, lp.BOUNDS
    for n, m in SIZES:
        kps, desc, points, S, row = bench_scene(lp, n, m, 60 + n)
        q = lp.query(0, S)
        want = lp.search(kps, desc, points, q, row, None, None, sf, bounds)
        out = {"features": n, "points": m, "occupied": int((row != -1).sum()), **{k: int(want[k]) for k in ("n_in_view", "n_matches", "n_researched", "n_total")}}
        cap = n + 8
        k2, d2, cell = np.zeros((1, cap), pkg.KP_DTYPE), np.zeros((1, cap, 32), np.uint8), np.full((1, cap), -1, np.int32)
        k2[0, :n], d2[0, :n], cell[0, :n] = kps, desc, lp.lr.grid_cells(kps, bounds)
        d_kps, d_desc, d_cell, d_counts, d_pts = up(k2), up(d2), up(cell), up(np.array([n], np.int32)), up(points)
        d_start = torch.zeros((1, 64 * 48 + 1), dtype=torch.int32, device="cuda")
        d_items = torch.full((1, cap), -1, dtype=torch.int32, device="cuda")
        mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), 1, cap, d_start.data_ptr(), d_items.data_ptr())
        for nq in (1, QUERIES):
            rows = np.full((nq, cap), -1, np.int32)
            rows[:, :n] = row
            d_rows = up(rows)
            d_loop = torch.zeros((nq, cap), dtype=torch.int32, device="cuda")
            d_stats = torch.zeros((nq, 8), dtype=torch.int32, device="cuda")
            queries = np.array([q] * nq, lp.QUERY)
            first, count = np.zeros(nq, np.int32), np.full(nq, m, np.int32)

            def call():
                mt.loop_points_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), 1,
                                            d_pts.data_ptr(), m, first, count, queries, d_rows.data_ptr(), d_loop.data_ptr(), d_stats.data_ptr(), cap, sf,
                                            bounds=bounds)
            out[f"device_ms_{nq}_queries"] = events(call)
            got = d_loop.cpu().numpy()
            assert all(np.array_equal(got[k, :n], want["loop_match"]) for k in range(nq)), "the timed call differs from the restatement"
        view = dict(keys_un=kps, desc=desc)
        out["host_form_ms"] = round(wall(lambda: mt.loop_points(view, points, q, sf, matched=row, bounds=bounds), reps), 4)
        kf, keep = hlb.standin(kps, desc, lp.INTR, sf, bounds)
        found, row_out, _, ms = hlb.search("dropin", kf, points, S, row, repeat=reps + 1)
        assert found == want["n_matches"] and np.array_equal(row_out, np.where(want["loop_match"] >= 0, want["loop_match"], row))
        out["dropin_ms"] = round(float(np.median(ms[1:])), 4)
        # the existing host class's search alone on the same scene: the queries are built outside the timed call
        shim = types.SimpleNamespace(WINDOW_QUERY=hb.WINDOW_QUERY,
                                     standin_predict_scale=lambda md, cd, _sf1, _nl: lp.lr.table_level(np.asarray(md, np.float32) / np.asarray(cd, np.float32), sf))
        cam = types.SimpleNamespace(fx=q["fx"], fy=q["fy"], cx=q["cx"], cy=q["cy"], mbf=0.0, min_x=bounds[0], max_x=bounds[1], min_y=bounds[2], max_y=bounds[3])
        Rcw, tcw, Ow = lp.decompose(S)
        with np.errstate(all="ignore"):
            wq, pos = ap.keyframe_queries(shim, cam, Rcw, tcw, Ow, points["pos"], points["normal"], points["min_distance"], points["max_distance"],
                                          points["desc"], np.arange(m), (points["flags"] & lp.SKIP) == 0, False, sf[1], len(sf))
        v, keep_v = hb.frame_view(kps, desc, None, tuple(float(b) for b in bounds))
        n_host, _ = hb.search_projection_sim("host", v, wq, row, sf, 10)
        assert n_host == want["n_matches"]
        out["host_class_ms"] = round(wall(lambda: hb.search_projection_sim("host", v, wq, row, sf, 10), reps), 4)
        print(json.dumps(out), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
