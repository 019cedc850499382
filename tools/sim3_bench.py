#!/usr/bin/env python3
"""Times ComputeSim3's Sim3Solver (SetRansacParameters(0.99, 20, 300); iterate(5) from a fresh state, and a whole find() with 300
iterations allowed) on synthetic keyframe pairs with 50, 150 and 500 correspondences, 40 % outliers, 0.5 px noise:
  - the resident path (amos_match_sim3_batch_device: one launch) between two HIP events on the matcher's stream, one pair per call and 8
    pairs per call (every pair its own two keyframe slots), medians of 30 calls after warm-up (every call resets the solver, so every
    call does the same work);
  - the host-compiled single-threaded solver over the same arithmetic (tests/host_sim3: amos_sim3_core.h as plain C++), constructor and
    the call, wall clock, median of 5;
  - the host form (amos_match_sim3 through OrbMatcher.sim3) and the C++ drop-in ORB_SLAM2::DeviceSim3Solver over it (std::chrono inside
    the harness around iterate), wall clock, medians of 5.
There is no figure for the reference's own class: it needs OpenCV, which is not here.  Prints one JSON line per size and mode
(milliseconds)."""
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
    import host_sim3_binding as hb
    import sim3_cases as sc
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

    for nc in (50, 150, 500):
        pairs = [sc.make_pair(nc, 0.4, 0.5, 300 + nc + k, n_features=nc + 40) for k in range(PAIRS)]
        n = len(pairs[0]["kps1"])
        cap = n + 8
        for mode, n_it in (("iterate5", 5), ("find", 300)):
            out = {"correspondences": nc, "features": n, "mode": mode}
            for npairs in (1, PAIRS):
                kps, pts = np.zeros((2 * npairs, cap), pkg.KP_DTYPE), np.zeros((2 * npairs, cap), pkg.SIM3_POINT_DTYPE)
                rows = np.full((npairs, cap), -1, np.int32)
                cams = np.zeros(2 * npairs, pkg.SIM3_CAMERA_DTYPE)
                for k in range(npairs):
                    p = pairs[k]
                    kps[2 * k, :n], kps[2 * k + 1, :n], pts[2 * k, :n], pts[2 * k + 1, :n] = p["kps1"], p["kps2"], p["points1"], p["points2"]
                    rows[k, :n] = p["match12"]
                    cams[2 * k:2 * k + 2] = hb.cameras_of(pkg, p)
                d_kps, d_pts, d_rows, d_counts = up(kps), up(pts), up(rows), up(np.full(2 * npairs, n, np.int32))
                d_1, d_2 = up(np.arange(0, 2 * npairs, 2, dtype=np.int32)), up(np.arange(1, 2 * npairs, 2, dtype=np.int32))
                d_state = torch.zeros((npairs, pkg.sim3_state_bytes(cap)), dtype=torch.uint8, device="cuda")
                d_res = torch.zeros((npairs, 160), dtype=torch.uint8, device="cuda")
                d_inl = torch.zeros((npairs, cap), dtype=torch.uint8, device="cuda")
                d_out = torch.zeros((npairs, cap), dtype=torch.int32, device="cuda")
                par = [pkg.sim3_params(1000 + k, reset=1, n_iterations=n_it, **sc.REFERENCE) for k in range(npairs)]

                def call():
                    mt.sim3_batch_device(d_kps.data_ptr(), d_counts.data_ptr(), d_pts.data_ptr(), cams, d_1.data_ptr(), d_2.data_ptr(), npairs,
                                         d_rows.data_ptr(), sc.LEVEL_SIGMA2, par, cap, d_state.data_ptr(), d_res.data_ptr(), d_inl.data_ptr(),
                                         d_out.data_ptr())
                out[f"device_ms_{npairs}_pairs"] = events(call)
                res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.SIM3_RESULT_DTYPE)
                out[f"iterations_{npairs}_pairs"] = [int(x) for x in res["iterations"]]
                out[f"inliers_{npairs}_pairs"] = [int(x) for x in res["n_inliers"]]
            p0 = pairs[0]
            par0 = pkg.sim3_params(1000, reset=1, n_iterations=n_it, **sc.REFERENCE)
            cams0 = hb.cameras_of(pkg, p0)

            def host_compiled():
                s = hb.HostSolver(pkg, p0["kps1"], p0["points1"], p0["kps2"], p0["points2"], cams0, p0["match12"], sc.LEVEL_SIGMA2, par0)
                r = s.iterate(n_it)
                s.close()
                return r
            r_host = host_compiled()[0]
            out["host_compiled_single_thread_ms"] = round(wall(host_compiled), 4)
            out["host_compiled_iterations"] = int(r_host["iterations"])
            out["host_form_ms"] = round(wall(lambda: mt.sim3(p0["kps1"], p0["points1"], p0["kps2"], p0["points2"], cams0, p0["match12"],
                                                             sc.LEVEL_SIGMA2, par0)), 4)
            objects, _ = sc.standin_objects(p0, moved=False)
            out["dropin_iterate_ms"] = round(float(np.median([hb.dropin(pkg, objects, sc.LEVEL_SIGMA2, 0, 1000, sc.REFERENCE, n_it, 1)[2]
                                                              for _ in range(5)])), 4)
            print(json.dumps(out), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
