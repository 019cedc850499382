"""Time of amos_frame_stereo_match_batch_device (Frame::ComputeStereoMatches on the device: k_stereo_match + k_stereo_median) per stereo pair,
on one handle holding 2 * P interleaved 640x480 synthetic frames (left, right, left, right ...; disparities 12 and 31), measured with HIP
events on the handle's stream -- and beside it the time of amos_orb_pyramid_images for two frames, the device-to-host transfer of both
pyramids that a host-side ComputeStereoMatches needs and this path does not.  Prints one JSON line.
Run it under `timeout`; for per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/stereo_bench.py`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    import stereo_restatement as sr
    pkg = entry.load_package()
    w, h, P = 640, 480, args.pairs
    frames = []
    for p in range(P):
        frames.extend(sr.stereo_pair(3 + p, h, w, 12, 31, 99 + p))
    ext = pkg.OrbExtractor(max_batch=2 * P)
    stream = torch.cuda.ExternalStream(ext.stream)
    d = torch.from_numpy(np.stack(frames)).cuda()
    ur = torch.zeros((P, ext.capacity), dtype=torch.float32, device="cuda")
    dep, sad = torch.zeros_like(ur), torch.zeros((P, ext.capacity), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.extract_batch_device(d.data_ptr(), h * w, w, w, h, 2 * P)
    ext.sync()
    counts = [len(ext.batch_fetch(f)[0]) for f in range(2 * P)]
    mbf, min_z = 40.0, 40.0 / 525.0
    out = {"pairs": P, "reps": args.reps, "width": w, "height": h, "keypoints_mean": round(float(np.mean(counts)), 1)}
    for n_pairs in sorted({1, P}):
        def call():
            ext.stereo_match_batch_device(None, n_pairs, mbf, min_z, ur.data_ptr(), dep.data_ptr(), sad.data_ptr())
        for _ in range(3):
            call()
        stream.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = []
        for _ in range(args.reps):
            ev[0].record(stream)
            call()
            ev[1].record(stream)
            ev[1].synchronize()
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
        key = f"match_{n_pairs}_pairs"
        out[key + "_us_median"] = round(float(np.median(times)), 1)
        out[key + "_us_min"] = round(float(np.min(times)), 1)
        out[key + "_us_per_pair"] = round(float(np.median(times)) / n_pairs, 1)
    out["kept_per_pair_mean"] = round(float((ur.cpu().numpy() >= 0).sum()) / P, 1)
    # the transfer the device path makes unnecessary: both pyramids of one pair to host memory (padded planes, as mvImagePyramid)
    lw, lh = ext.level_sizes(w, h)
    planes = [np.zeros((int(lh[l]) + 38, int(lw[l]) + 38), np.uint8) for l in range(ext.n_levels)]
    ptrs = (C.c_void_p * ext.n_levels)(*[pl.ctypes.data for pl in planes])
    strides = (C.c_size_t * ext.n_levels)(*[pl.strides[0] for pl in planes])
    times = []
    for rep in range(args.reps + 3):
        t0 = time.perf_counter()
        for f in (0, 1):
            rc = ext.L.amos_orb_pyramid_images(ext.h, f, ptrs, strides, 1)
            assert rc == 0, rc
        if rep >= 3:
            times.append((time.perf_counter() - t0) * 1e6)
    out["pyramid_download_2_frames_us_median"] = round(float(np.median(times)), 1)
    out["pyramid_download_2_frames_us_min"] = round(float(np.min(times)), 1)
    out["pyramid_bytes_2_frames"] = int(2 * sum(pl.size for pl in planes))
    ext.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
