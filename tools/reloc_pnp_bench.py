#!/usr/bin/env python3
"""Times Relocalization's PnPsolver (SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), iterate(5) from a fresh state) on synthetic pairs
with 50, 150 and 500 correspondences, 30 % outliers, 0.5 px noise:
  - the resident path (amos_match_reloc_pnp_batch_device: one launch) between two HIP events on the matcher's stream, one pair per call
    and 8 pairs on one frame per call, medians of 30 calls (every call resets the solver, so every call does the same work);
  - the host-compiled single-threaded solver over the same arithmetic (tests/host_reloc_pnp: amos_pnp_core.h as plain C++), constructor
    and iterate(5), wall clock, median of 5;
  - the host form (amos_match_reloc_pnp through OrbMatcher.reloc_pnp) and the C++ drop-in ORB_SLAM2::DevicePnPsolver over it (std::chrono
    inside the harness around iterate), wall clock, medians of 5.
There is no figure for the reference's own class: it needs OpenCV, which is not here.  Prints one JSON line per size (milliseconds)."""
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
    import host_reloc_pnp_binding as hp
    import reloc_pnp_cases as rc
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
        pairs = [rc.make_pair(nc, 0.3, 0.5, seed=100 + nc + k, n_features=nc + 104) for k in range(PAIRS)]
        n = len(pairs[0]["kps"])
        cap = n + 8
        out = {"correspondences": nc, "features": n}
        K = [np.float32(x) for x in pairs[0]["K"]]
        for npairs in (1, PAIRS):
            # one frame; pair k's features are its own scene's, so every pair gets a frame slot of its own
            kps, counts = np.zeros((npairs, cap), pkg.KP_DTYPE), np.full(npairs, n, np.int32)
            bow = np.full((npairs, cap), -1, np.int32)
            for k in range(npairs):
                kps[k, :n], bow[k, :n] = pairs[k]["kps"], pairs[k]["bow_match"]
            off = np.concatenate([[0], np.cumsum([len(p["points"]) for p in pairs[:npairs]])]).astype(np.int32)
            d_kps, d_counts, d_bow, d_pts = up(kps), up(counts), up(bow), up(np.concatenate([p["points"] for p in pairs[:npairs]]))
            d_state = torch.zeros((npairs, pkg.reloc_pnp_state_bytes(cap)), dtype=torch.uint8, device="cuda")
            d_res = torch.zeros((npairs, 104), dtype=torch.uint8, device="cuda")
            d_inl = torch.zeros((npairs, cap), dtype=torch.uint8, device="cuda")
            d_match = torch.zeros((npairs, cap), dtype=torch.int32, device="cuda")
            d_found = torch.zeros(int(off[-1]), dtype=torch.uint8, device="cuda")
            par = [pkg.reloc_pnp_params(K, 1000 + k, reset=1, n_iterations=5, **rc.REFERENCE) for k in range(npairs)]

            def call():
                mt.reloc_pnp_batch_device(d_kps.data_ptr(), d_counts.data_ptr(), npairs, d_pts.data_ptr(), list(range(npairs)), off, d_bow.data_ptr(),
                                          rc.LEVEL_SIGMA2, par, cap, d_state.data_ptr(), d_res.data_ptr(), d_inl.data_ptr(), d_match.data_ptr(),
                                          d_found.data_ptr())
            out[f"device_ms_{npairs}_pairs"] = events(call)
            res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.RELOC_PNP_RESULT_DTYPE)
            out[f"iterations_{npairs}_pairs"] = [int(x) for x in res["iterations"]]
            out[f"inliers_{npairs}_pairs"] = [int(x) for x in res["n_inliers"]]
        p0 = pairs[0]
        par0 = pkg.reloc_pnp_params(K, 1000, reset=1, n_iterations=5, **rc.REFERENCE)

        def host_compiled():
            s = hp.HostSolver(pkg, p0["kps"], p0["bow_match"], p0["points"], rc.LEVEL_SIGMA2, par0)
            r = s.iterate(5)
            s.close()
            return r
        r_host = host_compiled()[0]
        out["host_compiled_single_thread_ms"] = round(wall(host_compiled), 4)
        out["host_compiled_iterations"] = int(r_host["iterations"])
        out["host_form_ms"] = round(wall(lambda: mt.reloc_pnp(p0["kps"], p0["bow_match"], p0["points"], rc.LEVEL_SIGMA2, par0)), 4)
        bad = (p0["points"]["flags"] & 1).astype(np.uint8)
        out["dropin_iterate_ms"] = round(float(np.median([hp.dropin(pkg, p0["kps"], p0["K"], rc.LEVEL_SIGMA2, p0["points"]["pos"], bad, p0["bow_match"],
                                                                   1000, rc.REFERENCE, 5, 1)[1] for _ in range(5)])), 4)
        print(json.dumps(out), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
