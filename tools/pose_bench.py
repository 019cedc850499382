#!/usr/bin/env python3
"""Times Optimizer::PoseOptimization on synthetic frames (tests/pose_optimization_cases.py: mixed monocular / stereo edges, 25 % gross
outliers, a start 3 degrees / 5 cm off) with 200, 500 and 1 000 edges per frame:
  - device_ms_{1,32}_frames: amos_match_pose_optimization_batch_device (ONE launch) between two HIP events on the matcher's stream, frames
    resident, one frame and 32 frames per call, medians of 30 calls after 5 warm-up calls;
  - host_entry_ms: the one-frame host entry amos_match_pose_optimization, wall clock around the call (upload, launch, download, one
    synchronisation), median of 30;
  - dropin_ms: ORB_SLAM2::PoseOptimization on the stand-in frame (std::chrono inside tests/host_pose, mean of 5 runs on fresh objects,
    median of 5 such means): gathering, the host entry, the write-back and SetPose;
  - host_core_ms: amos_pose_core.h compiled for the host (g++ -O2, one thread) on the same frame, timed the same way.  It is the only host
    figure there is: g2o needs Eigen and cannot be built here, so nothing below compares against the reference's own optimiser.
Prints one JSON line per edge count (milliseconds)."""
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
    import host_pose_binding as hp
    import pose_optimization_cases as pc
    side = torch.cuda.Stream()  # the matcher issues on it, the events are recorded on it
    torch.cuda.set_stream(side)
    mt = pkg.OrbMatcher(stream=side.cuda_stream)
    for edges in (200, 500, 1000):
        c = pc.make_case(edges, "mixed", 0.25, seed=9)
        n = len(c["kps"])
        cap = n + 8
        out = {"edges": edges, "features": n}
        for nf in (1, 32):
            kps, ur, match = np.zeros((nf, cap), pkg.KP_DTYPE), np.full((nf, cap), -1, np.float32), np.full((nf, cap), -1, np.int32)
            kps[:, :n], ur[:, :n], match[:, :n] = c["kps"], c["u_right"], c["match"]

            def up(a):
                return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
            d_kps, d_ur, d_match, d_counts = up(kps), up(ur), up(match), up(np.full(nf, n, np.int32))
            d_pts = up(np.concatenate([c["pos"]] * nf))
            d_outlier = torch.zeros((nf, cap), dtype=torch.uint8, device="cuda")
            d_result = torch.zeros((nf, pkg.POSE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
            off = np.arange(nf + 1, dtype=np.int32) * len(c["pos"])
            cams = np.array([c["camera"]] * nf, pkg.POSE_CAMERA_DTYPE)
            times = []
            for rep in range(reps + 5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                mt.pose_optimization_batch_device(d_kps.data_ptr(), d_counts.data_ptr(), d_match.data_ptr(), d_pts.data_ptr(), off, cams, cap,
                                                  c["inv_sigma2"], d_outlier.data_ptr(), d_result.data_ptr(), d_u_right=d_ur.data_ptr())
                e1.record()
                e1.synchronize()
                if rep >= 5:
                    times.append(e0.elapsed_time(e1))
            mt.sync()
            res = np.frombuffer(d_result.cpu().numpy().tobytes(), pkg.POSE_RESULT_DTYPE)[0]
            out[f"device_ms_{nf}_frames"] = round(float(np.median(times)), 4)
            out["inliers"], out["iterations"], out["trials"] = int(res["n_inliers"]), int(res["iterations"].sum()), int(res["trials"].sum())
        times = []
        for rep in range(reps + 5):
            t0 = time.perf_counter()
            mt.pose_optimization(c["kps"], c["match"], c["pos"], c["camera"], c["inv_sigma2"], has_obs=c["has_obs"], u_right=c["u_right"])
            if rep >= 5:
                times.append((time.perf_counter() - t0) * 1e3)
        out["host_entry_ms"] = round(float(np.median(times)), 4)
        for which, key in (("dropin", "dropin_ms"), ("core", "host_core_ms")):
            hp.pose_optimization(which, c)
            out[key] = round(float(np.median([hp.pose_optimization(which, c, repeat=5)["ms"] for _ in range(5)])), 4)
        print(json.dumps(out), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
