"""Latency of amos_fmat_ransac_device (cv::findFundamentalMat(FM_RANSAC, 0.1, 0.99) on the device) on synthetic two-view scenes: one problem
of n = 1000 correspondences at 30 % and 60 % gross outliers, and a batch of 64 such problems in one launch.  Prints one JSON line.
Run it under `timeout`; for per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/fmat_bench.py`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    import fmat_restatement as fr
    pkg = entry.load_package()
    fm = pkg.FundamentalRansac(max_points=args.n, max_problems=args.batch)
    stream = torch.cuda.ExternalStream(fm.stream)
    out = {"n": args.n, "reps": args.reps}
    for frac in (0.3, 0.6):
        for nb in (1, args.batch):
            rng = np.random.default_rng(5)
            scenes = [fr.two_view(rng, args.n, frac, 0.02) for _ in range(nb)]  # noise well inside the 0.1 px threshold
            P1 = torch.from_numpy(np.concatenate([s[0] for s in scenes])).cuda()
            P2 = torch.from_numpy(np.concatenate([s[1] for s in scenes])).cuda()
            cnt = torch.full((nb,), args.n, dtype=torch.int32, device="cuda")
            off = torch.arange(nb, dtype=torch.int32, device="cuda") * args.n
            F = torch.zeros((nb, 9), dtype=torch.float64, device="cuda")
            st = torch.zeros((nb, 4), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def call():
                fm.ransac_device(nb, P1.data_ptr(), P2.data_ptr(), off.data_ptr(), cnt.data_ptr(), None, F.data_ptr(), st.data_ptr())
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
            s = st.cpu().numpy()
            key = f"out{int(frac * 100)}_batch{nb}"
            out[key + "_us_median"] = round(float(np.median(times)), 1)
            out[key + "_us_min"] = round(float(np.min(times)), 1)
            out[key + "_iterations_mean"] = round(float(s[:, 2].mean()), 1)
            out[key + "_all_models"] = bool((s[:, 0] == 1).all())
    fm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
