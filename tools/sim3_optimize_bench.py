#!/usr/bin/env python3
"""Times Optimizer::OptimizeSim3 on synthetic keyframe pairs (tests/sim3_optimization_cases.py: 25 % gross outliers, a start 3 degrees / 5 cm /
3 % off, the scale free) with 50, 150 and 400 correspondences per pair:
  - device_ms_{1,8}_pairs: amos_match_sim3_optimize_batch_device (ONE launch) between two HIP events on the matcher's stream, keyframes
    resident, one pair and eight pairs per call, medians of 30 calls after 5 warm-up calls;
  - host_entry_ms: the one-pair host entry amos_match_sim3_optimize, wall clock around the call (upload, launch, download, one
    synchronisation), median of 30;
  - dropin_ms: ORB_SLAM2::OptimizeSim3 on stand-in objects (std::chrono inside tests/host_sim3_optimize, the median of 9 runs on fresh
    objects): gathering, the host entry and the write-back;
  - host_core_ms: amos_sim3_opt_core.h compiled for the host (g++ -O2, one thread) on the same pair, timed the same way.  It is the only
    host figure there is: g2o needs Eigen and cannot be built here, so nothing below compares against the reference's own optimiser.
Prints one JSON line per correspondence count (milliseconds)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(reps=30):
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import host_sim3_optimize_binding as hso
    import sim3_optimization_cases as sc
    side = torch.cuda.Stream()  # the matcher issues on it, the events are recorded on it
    torch.cuda.set_stream(side)
    mt = pkg.OrbMatcher(stream=side.cuda_stream)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    for n in (50, 150, 400):
        s = sc.scene(n, 0, 0.25, seed=9)
        n1, n2 = len(s["kps1"]), len(s["kps2"])
        cap = max(n1, n2) + 8
        out = {"correspondences": n, "features_1": n1, "features_2": n2}
        for npairs in (1, 8):
            nf = 2 * npairs
            kps, pts = np.zeros((nf, cap), pkg.KP_DTYPE), np.zeros((nf, cap), pkg.SIM3_POINT_DTYPE)
            rows, counts = np.full((npairs, cap), -1, np.int32), np.zeros(nf, np.int32)
            for p in range(npairs):
                kps[2 * p, :n1], pts[2 * p, :n1], kps[2 * p + 1, :n2], pts[2 * p + 1, :n2] = s["kps1"], s["pts1"], s["kps2"], s["pts2"]
                rows[p, :n1], counts[2 * p], counts[2 * p + 1] = s["row"], n1, n2
            cams = np.array([s["cam1"], s["cam2"]] * npairs, pkg.SIM3_CAMERA_DTYPE)
            pairs = np.array([s["pair"]] * npairs, pkg.SIM3_OPT_PAIR_DTYPE)
            d_kps, d_pts, d_counts, d_rows = up(kps), up(pts), up(counts), up(rows)
            d_1, d_2 = up(np.arange(npairs, dtype=np.int32) * 2), up(np.arange(npairs, dtype=np.int32) * 2 + 1)
            d_out = torch.zeros((npairs, cap), dtype=torch.int32, device="cuda")
            d_result = torch.zeros((npairs, pkg.SIM3_OPT_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
            times = []
            for rep in range(reps + 5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                mt.sim3_optimize_batch_device(d_kps.data_ptr(), d_counts.data_ptr(), d_pts.data_ptr(), cams, d_1.data_ptr(), d_2.data_ptr(), pairs,
                                              d_rows.data_ptr(), d_out.data_ptr(), d_result.data_ptr(), cap, sc.INV_SIGMA2)
                e1.record()
                e1.synchronize()
                if rep >= 5:
                    times.append(e0.elapsed_time(e1))
            mt.sync()
            res = np.frombuffer(d_result.cpu().numpy().tobytes(), pkg.SIM3_OPT_RESULT_DTYPE)[0]
            out[f"device_ms_{npairs}_pairs"] = round(float(np.median(times)), 4)
            out["inliers"], out["iterations"], out["trials"] = int(res["n_inliers"]), int(res["iterations"].sum()), int(res["trials"].sum())
        times = []
        for rep in range(reps + 5):
            t0 = time.perf_counter()
            mt.sim3_optimize(s["kps1"], s["pts1"], s["kps2"], s["pts2"], [s["cam1"], s["cam2"]], s["row"], sc.INV_SIGMA2, s["pair"])
            if rep >= 5:
                times.append((time.perf_counter() - t0) * 1e3)
        out["host_entry_ms"] = round(float(np.median(times)), 4)
        for which, key in (("dropin", "dropin_ms"), ("core", "host_core_ms")):
            hso.optimize(which, s, sc.INV_SIGMA2)
            out[key] = round(float(np.median(hso.optimize(which, s, sc.INV_SIGMA2, repeat=9)["ms"])), 4)
        print(json.dumps(out), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
