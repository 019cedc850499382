#!/usr/bin/env python3
"""Times ComputeSim3's SearchBySim3 (ORBmatcher.cc:1314-1555, th = 7.5) on synthetic keyframe pairs of 500, 1 000 and 2 000 features at
640 x 480, about half the features with a map point and about a third of those already matched by the row:
  - the resident path (amos_match_sim3_search_batch_device: two memsets and two launches) between two HIP events on the matcher's stream,
    one pair per call and 8 pairs per call (one keyframe 1 against eight slots of keyframe 2, the loop closer's shape), medians of 30
    calls after warm-up;
  - the host form (amos_match_sim3_search through OrbMatcher.sim3_search) and the C++ drop-in ORB_SLAM2::SearchBySim3 over it
    (std::chrono inside the harness around the call, gathers and write-back included), wall clock, medians of 5;
  - the existing host class on the same scene (amos_host_search_by_sim3 of tests/host: the view-level search of ORBmatcher.h, one
    amos_match_list_distances call and a host loop; its two pre-filters are computed outside the timed call), wall clock, median of 5.
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

PAIRS = 8
TH = 7.5


def wall(fn, reps=5):
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms[1:]))


def bench_pair(ss, n, seed):
    """two keyframes of n features over one scene, s12 = 1 -> (kf1, kf2, cameras [2], PAIR record, row)"""
    import fuse_restatement as fr
    rng = np.random.default_rng(seed)
    sf = ss.SCALE.astype(np.float64)
    R2, t2 = ss.lr.pose(0.01, -0.015, 0.005, [0.06, -0.03, 0.04])
    pix = np.stack([rng.uniform(4, 636, n), rng.uniform(4, 476, n)], 1)
    depth = rng.uniform(2.0, 8.0, n)
    X = np.stack([(pix[:, 0] - ss.CX) / ss.FX * depth, (pix[:, 1] - ss.CY) / ss.FY * depth, depth], 1)
    level = rng.integers(0, len(sf), n)
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    order = [np.arange(n), rng.permutation(n)]
    kfs = []
    for f, (R, t) in enumerate(((np.eye(3), np.zeros(3)), (R2.astype(np.float64), t2.astype(np.float64)))):
        ids = order[f]
        q = X[ids] @ R.T + t
        u, v = ss.FX * q[:, 0] / q[:, 2] + ss.CX, ss.FY * q[:, 1] / q[:, 2] + ss.CY
        noise = rng.normal(0, 0.7, (n, 2)) * sf[level[ids], None]
        kps = np.zeros(n, ss.KP)
        kps["x"], kps["y"] = np.clip(u + noise[:, 0], 0.5, 639.4), np.clip(v + noise[:, 1], 0.5, 479.4)
        kps["octave"], kps["size"] = level[ids], 31
        desc = np.stack([fr.flip_bits(rng, base[i], int(rng.integers(0, 12))) for i in ids])
        pts = np.zeros(n, ss.MAP_POINT)
        pts["pos"] = X[ids]
        pts["max_distance"] = np.linalg.norm(q, axis=1) * sf[level[ids]] * rng.uniform(0.94, 0.98, n)
        pts["min_distance"] = pts["max_distance"] / sf[-1] / 1.5
        pts["flags"] = np.where(rng.random(n) < 0.5, 0, ss.lr.SKIP)
        pts["desc"] = np.stack([fr.flip_bits(rng, base[i], int(rng.integers(0, 12))) for i in ids])
        kfs.append(dict(kps=kps, desc=desc, points=pts))
    where2 = np.empty(n, np.int64)
    where2[order[1]] = np.arange(n)
    row = np.full(n, -1, np.int32)
    for i in range(n):
        j = where2[i]
        if kfs[0]["points"]["flags"][i] == 0 and rng.random() < 1 / 3:
            row[i] = j if kfs[1]["points"]["flags"][j] == 0 else ss.MATCHED_ELSEWHERE
    cams = np.array([ss.camera_of(np.eye(3), np.zeros(3)), ss.camera_of(R2, t2)], ss.CAMERA)
    R12 = R2.astype(np.float64).T
    pr = np.zeros((), ss.PAIR)
    pr["R12"], pr["t12"], pr["s12"], pr["th"], pr["enabled"] = R12.reshape(9), -R12 @ t2.astype(np.float64), 1.0, TH, 1
    return kfs[0], kfs[1], cams, pr, row


def main(reps=30):
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import adaptor_prefilter as ap
    import host_binding as hb
    import host_sim3_search_binding as hsb
    import sim3_search_restatement as ss
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

    sf, bounds = ss.SCALE, ss.BOUNDS
    for n in (500, 1000, 2000):
        kf1, kf2, cams2, pr, row = bench_pair(ss, n, 40 + n)
        want = ss.search(kf1, kf2, cams2[0], cams2[1], pr["R12"], pr["t12"], pr["s12"], TH, row, sf, bounds)
        out = {"features": n, "points_1": int((kf1["points"]["flags"] == 0).sum()), "points_2": int((kf2["points"]["flags"] == 0).sum()),
               "row_entries": int((row != -1).sum()), "n_found": want["stats"]["n_found"], "n_single_12": want["stats"]["n_single_12"],
               "n_single_21": want["stats"]["n_single_21"]}
        cap, nf = n + 8, PAIRS + 1
        kps, desc, pts = np.zeros((nf, cap), pkg.KP_DTYPE), np.zeros((nf, cap, 32), np.uint8), np.zeros((nf, cap), pkg.MAP_POINT_DTYPE)
        cell = np.full((nf, cap), -1, np.int32)
        cams = np.zeros(nf, pkg.SIM3_CAMERA_DTYPE)
        for f in range(nf):
            kf = kf1 if f == 0 else kf2
            kps[f, :n], desc[f, :n], pts[f, :n], cams[f] = kf["kps"], kf["desc"], kf["points"], cams2[min(f, 1)]
            cell[f, :n] = ss.lr.grid_cells(kf["kps"], bounds)
        d_kps, d_desc, d_pts, d_cell, d_counts = up(kps), up(desc), up(pts), up(cell), up(np.full(nf, n, np.int32))
        d_start = torch.zeros((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
        d_items = torch.full((nf, cap), -1, dtype=torch.int32, device="cuda")
        mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), nf, cap, d_start.data_ptr(), d_items.data_ptr())
        for npairs in (1, PAIRS):
            rows = np.full((npairs, cap), -1, np.int32)
            rows[:, :n] = row
            d_rows, d_out = up(rows), torch.zeros((npairs, cap), dtype=torch.int32, device="cuda")
            d_m1, d_m2 = torch.zeros((npairs, cap), dtype=torch.int32, device="cuda"), torch.zeros((npairs, cap), dtype=torch.int32, device="cuda")
            d_stats = torch.zeros((npairs, 8), dtype=torch.int32, device="cuda")
            d_1, d_2 = up(np.zeros(npairs, np.int32)), up(np.arange(1, npairs + 1, dtype=np.int32))
            records = np.array([pr] * npairs)

            def call():
                mt.sim3_search_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(),
                                            d_pts.data_ptr(), cams, d_1.data_ptr(), d_2.data_ptr(), records, d_rows.data_ptr(), d_out.data_ptr(),
                                            d_m1.data_ptr(), d_m2.data_ptr(), d_stats.data_ptr(), cap, sf, bounds=bounds)
            out[f"device_ms_{npairs}_pairs"] = events(call)
            got = d_out.cpu().numpy()
            assert all(np.array_equal(got[k, :n], want["match_out"]) for k in range(npairs)), "the timed call differs from the restatement"
        v1, v2 = dict(keys_un=kf1["kps"], desc=kf1["desc"]), dict(keys_un=kf2["kps"], desc=kf2["desc"])
        out["host_form_ms"] = round(wall(lambda: mt.sim3_search(v1, kf1["points"], v2, kf2["points"], cams2, pr, sf, row, bounds=bounds)), 4)
        s1, keep1 = hsb.standin(kf1, cams2[0], sf, bounds)
        s2, keep2 = hsb.standin(kf2, cams2[1], sf, bounds)
        found, row_out, ms = hsb.dropin(s1, s2, row, pr["R12"], pr["t12"], pr["s12"], TH, repeat=6)
        assert found == want["stats"]["n_found"] and np.array_equal(row_out, want["match_out"])
        out["dropin_ms"] = round(float(np.median(ms[1:])), 4)
        # the existing host class on the same scene: the queries of both directions are built outside the timed call
        shim = types.SimpleNamespace(WINDOW_QUERY=hb.WINDOW_QUERY,
                                     standin_predict_scale=lambda md, cd, _sf1, _nl: ss.lr.table_level(np.asarray(md, np.float32) / np.asarray(cd, np.float32), sf))
        cam_ns = types.SimpleNamespace(fx=ss.FX, fy=ss.FY, cx=ss.CX, cy=ss.CY, min_x=bounds[0], max_x=bounds[1], min_y=bounds[2], max_y=bounds[3])
        c12, c21 = ap.sim3_hops(pr["s12"], pr["R12"], pr["t12"])
        queries = []
        for kf, cam, hop, matched in ((kf1, cams2[0], c21, want["matched"][0]), (kf2, cams2[1], c12, want["matched"][1])):
            T = np.eye(4, dtype=np.float32)
            T[:3, :3], T[:3, 3] = cam["Rcw"].reshape(3, 3), cam["tcw"]
            p = kf["points"]
            with np.errstate(all="ignore"):
                queries.append(ap.sim3_direction(shim, cam_ns, cam_ns, T, hop, p["pos"], p["min_distance"], p["max_distance"], p["desc"], np.arange(n),
                                                 (p["flags"] == 0) & ~matched, sf[1], len(sf)))
        w1, k1 = hb.frame_view(kf1["kps"], kf1["desc"], None, bounds)
        w2, k2 = hb.frame_view(kf2["kps"], kf2["desc"], None, bounds)
        found_host, _ = hb.search_sim3("host", w1, w2, queries[0], queries[1], sf, sf, TH)
        assert found_host == want["stats"]["n_found"]
        out["host_class_ms"] = round(wall(lambda: hb.search_sim3("host", w1, w2, queries[0], queries[1], sf, sf, TH)), 4)
        print(json.dumps(out), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
