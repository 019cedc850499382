#!/usr/bin/env python3
"""Times the search of Tracking::TrackWithMotionModel on 640x480 synthetic frames with 500, 1 000 and 2 000 last-frame points per frame:
  - the resident path (amos_match_motion_model_batch_device: three launches, five with the second search) with HIP events on the matcher's
    stream, one frame and 32 frames per call, medians of 30 calls, once with retry_below = 0 and once with the second search forced on
    every frame (retry_below above any match count);
  - beside it, for the same points of one frame, the chain Tracking had before (fill, ORBmatcherFor::SearchByProjection(CurrentFrame,
    LastFrame, th, bMono): host projection and enumeration, one upload + distance kernel + download, host greedy loop and histogram; again
    with 2 * th below 20 matches) and the C++ drop-in over the host form, both wall clock (std::chrono inside the harness, mean of 5 runs on
    fresh objects, median of 5 such means), NOT event-timed.  Both start with the stand-in objects built; the drop-in's time is everything
    SearchByMotionModel does: gathering the arrays from the objects, the host form's upload, grid build, launches, download,
    synchronisation and the write-back.
Prints one JSON line per configuration (medians in milliseconds, and the share of projected points whose window was searched twice)."""
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
    import host_motion_binding as hm
    import local_points_restatement as lr
    import motion_model_restatement as mr
    import oracle_binding as ob
    orc = ob.Oracle(1000, 1.2, 8)
    k0, d0 = orc.extract(synth.frame(3, 0))
    k1, d1 = orc.extract(synth.frame(3, 1))
    sf, bounds, intr = orc.tables()["scale"], (0.0, 640.0, 0.0, 480.0), (520.0, 520.0, 320.0, 240.0)
    last = mr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1])
    cur = mr.moved(last, **mr.MOTIONS["sideways"])
    n, cap = len(k0), len(k0) + 8
    side = torch.cuda.Stream()  # the matcher issues on it, the events are recorded on it
    torch.cuda.set_stream(side)
    mt = pkg.OrbMatcher(stream=side.cuda_stream)
    for m in (500, 1000, 2000):
        rng = np.random.default_rng(m)
        pick = rng.integers(0, len(k1), m)  # the last frame as the harness needs it: point i belongs to last-frame feature i
        pts = mr.make_last_points(rng, k1[pick], d1[pick], m, last, intr, replace=False)
        out = {"points_per_frame": m, "features": n}
        for nf in (1, 32):
            kps, desc = np.zeros((nf, cap), pkg.KP_DTYPE), np.zeros((nf, cap, 32), np.uint8)
            cell = np.full((nf, cap), -1, np.int32)
            kps[:, :n], desc[:, :n], cell[:, :n] = k0, d0, lr.grid_cells(k0, bounds)

            def up(a):
                return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
            d_kps, d_desc, d_cell, d_counts = up(kps), up(desc), up(cell), up(np.full(nf, n, np.int32))
            d_pts = up(np.concatenate([pts] * nf))
            d_start = torch.zeros((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
            d_items = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
            d_query = torch.zeros((nf * m, 56), dtype=torch.uint8, device="cuda")
            d_projected = torch.zeros(nf * m, dtype=torch.uint8, device="cuda")
            d_match = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
            d_stats = torch.zeros((nf, 8), dtype=torch.int32, device="cuda")
            mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), nf, cap, d_start.data_ptr(), d_items.data_ptr())
            off = np.arange(nf + 1, dtype=np.int32) * m
            for label, retry_below in (("", 0), ("_second_search", 1 << 30)):
                cams = np.array([mr.camera(*cur, *last, *intr, th=15.0, retry_below=retry_below)] * nf, mr.CAMERA)
                times = []
                for rep in range(reps + 5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    mt.motion_model_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(),
                                                 d_pts.data_ptr(), off, cams, cap, sf, d_query.data_ptr(), d_projected.data_ptr(),
                                                 d_match.data_ptr(), d_stats.data_ptr(), bounds=bounds)
                    e1.record()
                    e1.synchronize()
                    if rep >= 5:
                        times.append(e0.elapsed_time(e1))
                mt.sync()
                st = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.MOTION_STATS_DTYPE)[0]
                out[f"device_ms_{nf}_frames{label}"] = round(float(np.median(times)), 4)
                if not label:
                    out["projected"], out["matches"] = int(st["n_projected"]), int(st["n_matches"])
                    out["researched_share"] = round(float(st["n_researched"]) / max(int(st["n_projected"]), 1), 4)
        cam = mr.camera(*cur, *last, *intr, th=15.0)
        for which in ("parent", "dropin"):
            ms = [hm.search_motion_model(which, k0, d0, None, k1[pick], pts, cam, sf, bounds, repeat=5)["ms"] for _ in range(5)]
            out[f"{which}_host_ms"] = round(float(np.median(ms)), 4)
        print(json.dumps(out), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
