#!/usr/bin/env python3
"""Times step 2 of Tracking::SearchLocalPoints on 640x480 synthetic frames with 1 000, 2 000 and 4 000 map points per frame:
  - the resident path (amos_match_local_points_batch_device: three launches) with HIP events, one frame and 32 frames per call;
  - beside it, for the same queries of one frame, the chain the host classes had before (isInFrustum in C++ on the host, then
    ORBmatcherFor::SearchByProjection: host enumeration, one distance call, host greedy loop) and the C++ drop-in over the host form, both
    wall clock (std::chrono inside the harness, mean of 5 runs on fresh objects, median of 5 such means), NOT event-timed.  Both start
    with the stand-in objects built: the parent's time is its isInFrustum loop and the search (host enumeration, one upload + distance
    kernel + download, host greedy loop); the drop-in's time is everything SearchLocalPoints does -- gathering the arrays from the objects
    (cv::Mat clones of GetWorldPos / GetNormal / GetDescriptor per point), the host form's upload, grid build, three launches, download
    and synchronisation, and the write-back.
Prints one JSON line per configuration (medians in milliseconds, and the share of points in view whose window was searched twice)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(reps=30):
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import importlib
    synth = importlib.import_module("amos_slam_amd.synth")
    import host_local_binding as hl
    import local_points_restatement as lr
    import oracle_binding as ob
    orc = ob.Oracle(1000, 1.2, 8)
    k0, d0 = orc.extract(synth.frame(3, 0))
    k1, d1 = orc.extract(synth.frame(3, 1))
    sf, bounds = orc.tables()["scale"], (0.0, 640.0, 0.0, 480.0)
    cam = lr.camera(*lr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1]), 520.0, 520.0, 320.0, 240.0, th=1.0)
    n, cap = len(k0), len(k0) + 8
    side = torch.cuda.Stream()  # the matcher issues on it, the events are recorded on it
    torch.cuda.set_stream(side)
    mt = pkg.OrbMatcher(stream=side.cuda_stream)
    for m in (1000, 2000, 4000):
        pts = lr.make_points(np.random.default_rng(m), k1, d1, m, cam, sf)
        out = {"points_per_frame": m, "features": n}
        for nf in (1, 32):
            kps, desc = np.zeros((nf, cap), pkg.KP_DTYPE), np.zeros((nf, cap, 32), np.uint8)
            cell = np.full((nf, cap), -1, np.int32)
            kps[:, :n], desc[:, :n], cell[:, :n] = k0, d0, lr.grid_cells(k0, bounds)

            def up(a):
                return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
            d_kps, d_desc, d_cell, d_counts = up(kps), up(desc), up(cell), up(np.full(nf, n, np.int32))
            d_occ, d_pts = torch.zeros(nf * cap, dtype=torch.uint8, device="cuda"), up(np.concatenate([pts] * nf))
            d_start = torch.zeros((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
            d_items = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
            d_query = torch.zeros((nf * m, 56), dtype=torch.uint8, device="cuda")
            d_in_view = torch.zeros(nf * m, dtype=torch.uint8, device="cuda")
            d_match = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
            d_stats = torch.zeros((nf, 4), dtype=torch.int32, device="cuda")
            mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), nf, cap, d_start.data_ptr(), d_items.data_ptr())
            off, cams = np.arange(nf + 1, dtype=np.int32) * m, np.array([cam] * nf, lr.CAMERA)
            times = []
            for rep in range(reps + 5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                mt.local_points_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(),
                                             d_pts.data_ptr(), off, cams, d_occ.data_ptr(), cap, sf, d_query.data_ptr(), d_in_view.data_ptr(),
                                             d_match.data_ptr(), d_stats.data_ptr(), bounds=bounds)
                e1.record()
                e1.synchronize()
                if rep >= 5:
                    times.append(e0.elapsed_time(e1))
            mt.sync()
            st = d_stats.cpu().numpy()[0]
            out[f"device_ms_{nf}_frames"] = round(float(np.median(times)), 4)
            out["in_view"], out["matches"], out["researched_share"] = int(st[0]), int(st[1]), round(float(st[2]) / max(int(st[0]), 1), 4)
        occupant = np.full(n, -1, np.int32)
        for which in ("parent", "dropin"):
            ms = [hl.search_local_points(which, k0, d0, None, pts, cam, occupant, sf, bounds, repeat=5)["ms"] for _ in range(5)]
            out[f"{which}_host_ms"] = round(float(np.median(ms)), 4)
        print(json.dumps(out), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
