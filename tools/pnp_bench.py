"""Latency of amos_pnp_ransac_device (cv::solvePnPRansac(SOLVEPNP_P3P, 500, 0.4, 0.98) + EPnP refit on the device) on synthetic scenes: one
problem of n = 1000 correspondences at 30 % and 60 % gross outliers, and a batch of 64 such problems in one launch.  Prints one JSON line.
The per-round time and the fixed part (load, final mask, EPnP refit) are derived from the two outlier fractions, which run different
numbers of 64-iteration rounds.  Run it under `timeout`; for per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python tools/pnp_bench.py`."""
import argparse
import json
import math
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
    import pnp_restatement as pr
    pkg = entry.load_package()
    pnp = pkg.PnpRansac(max_points=args.n, max_problems=args.batch)
    stream = torch.cuda.ExternalStream(pnp.stream)
    out = {"n": args.n, "reps": args.reps}
    for frac in (0.3, 0.6):
        for nb in (1, args.batch):
            rng = np.random.default_rng(5)
            scenes = [pr.scene(rng, args.n, frac, 0.05) for _ in range(nb)]
            O = torch.from_numpy(np.concatenate([s[0] for s in scenes])).cuda()
            I = torch.from_numpy(np.concatenate([s[1] for s in scenes])).cuda()
            cnt = torch.full((nb,), args.n, dtype=torch.int32, device="cuda")
            off = torch.arange(nb, dtype=torch.int32, device="cuda") * args.n
            Rt = torch.zeros((nb, 12), dtype=torch.float64, device="cuda")
            st = torch.zeros((nb, 5), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def call():
                pnp.ransac_device(nb, O.data_ptr(), I.data_ptr(), off.data_ptr(), cnt.data_ptr(), None, *pr.K_TUM, Rt.data_ptr(), st.data_ptr())
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
            out[key + "_rounds_max"] = int(max(math.ceil(v / 64) for v in s[:, 2]))
            out[key + "_all_refit"] = bool((s[:, 0] == 1).all() and (s[:, 4] == 1).all())
    r30, r60 = out["out30_batch1_rounds_max"], out["out60_batch1_rounds_max"]
    if r60 > r30:
        per_round = (out["out60_batch1_us_median"] - out["out30_batch1_us_median"]) / (r60 - r30)
        out["per_round_us"] = round(per_round, 1)
        out["fixed_us"] = round(out["out30_batch1_us_median"] - r30 * per_round, 1)
    pnp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
