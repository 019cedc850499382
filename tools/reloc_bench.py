#!/usr/bin/env python3
"""Times Relocalization's SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) on 640x480 synthetic frames with 500, 1 000 and
2 000 keyframe points against a frame of as many features, a third of them set on entry and a fifth of the points found, for
(th, ORBdist) = (10, 100) and (3, 64):
  - the resident path (amos_match_reloc_batch_device: three launches) with HIP events on the matcher's stream, one pair per call and 8
    pairs on one frame per call, medians of 30 calls; d_match is restored ahead of every call, outside the timed window;
  - the host form (amos_match_reloc through OrbMatcher.reloc) and the C++ drop-in SearchByProjection<Frame, KeyFrame, MapPoint> over it
    (std::chrono inside the harness, mean of 5 runs on fresh objects), wall clock, medians of 5;
  - the host class's loop on the same inputs (hb.search_kf("host", ...) on the projected records: enumeration, one upload + distance kernel +
    download, host greedy loop and histogram; the host projection of the adaptor is not in it), wall clock, median of 5;
  - the chain pose optimisation -> search -> pose optimisation on a frame whose points are its own features, 120 of them matched on
    entry: resident (three calls, HIP events, no host step) and through the host forms (three synchronous calls, wall clock).
Prints one JSON line per configuration (medians in milliseconds)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PAIRS = 8


def wall(fn, reps=5):
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms[1:]))


def main(reps=30):
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import importlib
    synth = importlib.import_module("amos_slam_amd.synth")
    import host_binding as hb
    import host_reloc_binding as hrb
    import local_points_restatement as lr
    import motion_model_restatement as mr
    import oracle_binding as ob
    import pose_optimization_cases as pc
    import reloc_restatement as rr
    bounds, intr = (0.0, 640.0, 0.0, 480.0), (520.0, 520.0, 320.0, 240.0)
    side = torch.cuda.Stream()  # the matcher issues on it, the events are recorded on it
    torch.cuda.set_stream(side)
    mt = pkg.OrbMatcher(stream=side.cuda_stream)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def events(call, restore):
        times = []
        for rep in range(reps + 5):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if rep >= 5:
                times.append(e0.elapsed_time(e1))
        mt.sync()
        return round(float(np.median(times)), 4)

    for m in (500, 1000, 2000):
        orc = ob.Oracle(m, 1.2, 8)
        k0, d0 = orc.extract(synth.frame(3, 0))
        k1, d1 = orc.extract(synth.frame(3, 1))
        sf = orc.tables()["scale"]
        inv_sigma2 = (np.float32(1.0) / (sf * sf)).astype(np.float32)
        n, cap = len(k0), len(k0) + 8
        rng = np.random.default_rng(m)
        pts = rr.make_points(rng, k1, d1, m, rr.KF_POSE, intr, sf)
        match_in, found = rr.entry_state(rng, n, m)
        cur = mr.moved(rr.KF_POSE, **rr.CUR_MOTIONS[0])
        kps, desc, cell = np.zeros((1, cap), pkg.KP_DTYPE), np.zeros((1, cap, 32), np.uint8), np.full((1, cap), -1, np.int32)
        kps[0, :n], desc[0, :n], cell[0, :n] = k0, d0, lr.grid_cells(k0, bounds)
        d_kps, d_desc, d_cell, d_counts = up(kps), up(desc), up(cell), up(np.array([n], np.int32))
        d_start = torch.zeros((1, 64 * 48 + 1), dtype=torch.int32, device="cuda")
        d_items = torch.zeros((1, cap), dtype=torch.int32, device="cuda")
        mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), 1, cap, d_start.data_ptr(), d_items.data_ptr())
        row = np.full(cap, -1, np.int32)
        row[:n] = match_in
        # stand-in objects of the drop-in: keyframe feature i carries point i
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = cur[0], cur[1]
        kk = np.zeros(m, hb.KP)
        kk[:] = k1[np.arange(m) % len(k1)]
        kk["angle"] = pts["angle"]
        t_pts, keep0 = hb.test_points(pts["pos"], np.zeros((m, 3), np.float32), pts["desc"], ((pts["flags"] & rr.HAS_OBS) != 0).astype(np.int32),
                                      (pts["flags"] & rr.SKIP).astype(np.uint8), pts["min_distance"], pts["max_distance"])
        t_kf, keep1 = hb.test_kf(hb.test_camera(np.eye(4), sf, *intr, 0.0, 0.0, bounds=bounds), kk, np.zeros((m, 32), np.uint8), None, np.arange(m, dtype=np.int32))
        t_cur, keep2 = hb.test_kf(hb.test_camera(T, sf, *intr, 0.0, 0.0, bounds=bounds), k0, d0, None, np.where(match_in >= 0, 0, -1).astype(np.int32))
        view, keep3 = hb.frame_view(k0, d0, None, bounds)
        for th, orb_dist in rr.PARAMS:
            out = {"points": m, "features": n, "th": th, "orb_dist": orb_dist}
            cam = rr.camera(*cur, *intr, th=th, orb_dist=orb_dist)
            for npairs in (1, PAIRS):
                d_pts, d_found = up(np.concatenate([pts] * npairs)), up(np.concatenate([found] * npairs))
                d_match0, d_match = up(np.stack([row] * npairs)), up(np.stack([row] * npairs))
                d_query = torch.zeros((npairs * m, 48), dtype=torch.uint8, device="cuda")
                d_projected = torch.zeros(npairs * m, dtype=torch.uint8, device="cuda")
                d_stats = torch.zeros((npairs, 8), dtype=torch.int32, device="cuda")
                off, cams = np.arange(npairs + 1, dtype=np.int32) * m, np.array([cam] * npairs, rr.CAMERA)

                def call():
                    mt.reloc_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), 1,
                                          d_pts.data_ptr(), [0] * npairs, off, cams, cap, sf, d_query.data_ptr(), d_projected.data_ptr(),
                                          d_match.data_ptr(), d_stats.data_ptr(), bounds=bounds, d_found=d_found.data_ptr())
                out[f"device_ms_{npairs}_pairs"] = events(call, lambda: d_match.copy_(d_match0))
                st = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.RELOC_STATS_DTYPE)[0]
                if npairs == 1:
                    out.update(projected=int(st["n_projected"]), matches=int(st["n_matches"]), occupied=int(st["n_occupied"]),
                               researched_share=round(float(st["n_researched"]) / max(int(st["n_projected"]), 1), 4))
            out["host_form_ms"] = round(wall(lambda: mt.reloc(k0, d0, pts, cam, sf, match_in, found=found, bounds=bounds)), 4)
            out["dropin_ms"] = round(float(np.median([hrb.search_reloc(t_cur, t_kf, t_pts, found, th, orb_dist, True, repeat=5)[2] for _ in range(5)])), 4)
            q, projected, _, _ = rr.project(pts, cam, rr.found_of(pts, cam, found, match_in), sf, bounds)
            queries = q[projected == 1]
            host_n = hb.search_kf("host", view, queries, match_in, sf, th, orb_dist)[0]
            out["host_class_loop_ms"] = round(wall(lambda: hb.search_kf("host", view, queries, match_in, sf, th, orb_dist)), 4)
            out["host_class_matches"] = int(host_n)
            print(json.dumps(out), flush=True)
        # the chain: the points are the frame's own features seen from the true pose, 120 matched on entry, ten of them wrongly
        own = rr.make_points(rng, k0, d0, n, rr.KF_POSE, intr, sf, skip_share=0.0, behind=False)
        m_in = np.full(n, -1, np.int32)
        edges = rng.permutation(n)[:120]
        m_in[edges] = edges
        m_in[edges[:10]] = rng.integers(0, n, 10)
        Rs, ts = mr.moved(rr.KF_POSE, rx=0.004, ry=-0.003, rz=0.002, t=(0.01, -0.008, 0.006))
        start = pc.camera(Rs, ts, *intr, 20.0)
        rcam = rr.camera(Rs, ts, *intr, th=10.0, orb_dist=100, found_from_match=1)
        row[:n] = m_in
        d_own, d_match0, d_match = up(own), up(row), up(row)
        d_query = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
        d_projected = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_stats = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
        d_outlier = torch.zeros((1, cap), dtype=torch.uint8, device="cuda")
        d_res = torch.zeros((2, pkg.POSE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        off = np.array([0, n], np.int32)
        pose_kw = dict(point_stride=64, flags_offset=24, has_obs_bit=pkg.RELOC_POINT_HAS_OBS, clear_outliers=True)
        starts = np.array([start], pkg.POSE_CAMERA_DTYPE)

        def chain():
            for k in range(2):
                mt.pose_optimization_batch_device(d_kps.data_ptr(), d_counts.data_ptr(), d_match.data_ptr(), d_own.data_ptr(), off, starts, cap,
                                                  inv_sigma2, d_outlier.data_ptr(), d_res[k].data_ptr(), **pose_kw)
                if k == 0:
                    mt.reloc_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), 1,
                                          d_own.data_ptr(), [0], off, np.array([rcam], rr.CAMERA), cap, sf, d_query.data_ptr(),
                                          d_projected.data_ptr(), d_match.data_ptr(), d_stats.data_ptr(), bounds=bounds, d_pose=d_res[0].data_ptr())
        out = {"points": n, "features": n, "chain": "pose -> search(10, 100) -> pose", "edges_on_entry": 120}
        out["device_ms"] = events(chain, lambda: d_match.copy_(d_match0))
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.POSE_RESULT_DTYPE)
        out["inliers"] = [int(res["n_inliers"][0]), int(res["n_inliers"][1])]
        has_obs = ((own["flags"] & rr.HAS_OBS) != 0).astype(np.uint8)

        def host_chain():
            r1, o1, m1 = mt.pose_optimization(k0, m_in, own["pos"], start, inv_sigma2, has_obs=has_obs, clear_outliers=True)
            c2 = rr.camera(r1["Tcw"].reshape(3, 4)[:, :3], r1["Tcw"].reshape(3, 4)[:, 3], *intr, th=10.0, orb_dist=100, found_from_match=1)
            _, _, m2, _ = mt.reloc(k0, d0, own, c2, sf, m1, bounds=bounds)
            mt.pose_optimization(k0, m2, own["pos"], start, inv_sigma2, outlier=o1, has_obs=has_obs, clear_outliers=True)
        out["host_forms_ms"] = round(wall(host_chain), 4)
        print(json.dumps(out), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
