#!/usr/bin/env python3
"""Times ORBmatcher::Fuse as LocalMapping::SearchInNeighbors calls it, on the seeded stand-in maps of tests/host_fuse_binding.py:
  - neighbours: the map points of the current keyframe (0.6 x features of them) fused into 10 / 20 / 40 target keyframes of 500 / 1 000 / 2 000
    features.  dropin_ms: ONE ORB_SLAM2::FuseInNeighbors call (KeyFrameFuse.h: gather, one upload, one launch, one download, the write-backs
    and the host re-searches); parent_ms: the host class ORBmatcherFor::Fuse once per target on the same objects -- what the mapping thread ran
    before.  Two maps: "mixed": of the features a list point lands on, 80 % are empty, 8 % held by a point with more observations, 8 % by
    one with fewer (the list point survives with a new descriptor and is searched again on the host in every later target: host_researches)
    and 4 % by a bad point; "few_survivors": 88 / 8 / 0 / 4 %: a list point takes a new descriptor only once it has gathered more
    observations than the 10-observation occupant it meets.  Wall clock inside the harness (std::chrono) around the calls alone; every run
    starts from a freshly built map.
  - single: the one large call, 5 000 / 20 000 candidate points into one keyframe of 1 000 features, drop-in against host class alike.
  - device_ms: amos_match_fuse_batch_device alone on resident keyframes of 1 000 features and a shared list of 1 000 points, 1 pair and 32
    pairs, HIP events on the matcher's stream.
Each figure is the median of `reps` runs after `warm` warm-up runs.  Prints one JSON line per configuration (milliseconds)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(reps=15, warm=3):
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import fuse_restatement as fr
    import host_fuse_binding as fb
    import test_gpu_fuse as tg

    def med(ms):
        return round(float(np.median(ms[warm:])), 4)

    def both(m, targets, lst):
        r = {}
        for which in ("dropin", "parent"):
            res = fb.fuse_neighbors(which, m, targets, lst, repeat=reps + warm)
            r[f"{which}_ms"] = med(res["ms"])
            r[f"{which}_fused"] = int(res["n_fused"].sum())
            if which == "dropin":
                r["host_researches"] = int(res["n_host_searches"])
                r["dropin_search_ms"] = round(float(res["search_ms"]), 4)  # of the last run: the device call + the host re-searches
        assert r["dropin_fused"] == r["parent_fused"], r
        return r

    for mix, kinds in (("mixed", (0.8, 0.08, 0.08, 0.04)), ("few_survivors", (0.88, 0.08, 0.0, 0.04))):
        for nfeat in (500, 1000, 2000):
            for nt in (10, 20, 40):
                m, targets, lst = fb.neighbors_map(nfeat + nt, n_targets=nt, n_feat=nfeat, n_list=int(0.6 * nfeat), decoys=0, kinds=kinds)
                print(json.dumps(dict(case="neighbours", mix=mix, targets=nt, features=nfeat, points=len(lst), **both(m, targets, lst))), flush=True)
    for npts in (5000, 20000):
        m, targets, lst = fb.single_map(npts, n_feat=1000, n_points=npts)
        print(json.dumps(dict(case="single", features=1000, points=npts, **both(m, targets, lst))), flush=True)

    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    rng = np.random.default_rng(7)
    eye = np.eye(3, dtype=np.float32)
    for n_pairs in (1, 32):
        cam = fr.camera(eye, [0, 0, 0])
        kfs = [fr.make_keyframe(rng, 1000, 0) for _ in range(n_pairs)]
        points = fr.points_of(rng, kfs[0], 1000, cam)
        pairs = [(p, 0, 1000, 1000 * p, cam) for p in range(n_pairs)]
        sc = dict(kfs=kfs, points=points, pairs=pairs, skip=np.zeros(1000 * n_pairs, np.uint8), n_out=1000 * n_pairs, sf=fr.SCALE,
                  inv_sigma2=fr.INV_SIGMA2, bounds=fr.BOUNDS)
        res = tg.Resident(pkg, sc, stream=side.cuda_stream)
        bufs = res.alloc(n_pairs)
        times = []
        for rep in range(reps + warm):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res.launch(bufs, pairs, fr.LOCAL, True)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        out = res.fetch(bufs)
        print(json.dumps(dict(case="device", pairs=n_pairs, features=1000, points=1000, device_ms=med(times), in_view=int(out[4]["n_in_view"].sum()),
                              accepted=int(out[4]["n_accepted"].sum()))), flush=True)
        res.mt.close()


if __name__ == "__main__":
    main()
