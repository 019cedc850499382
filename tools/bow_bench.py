#!/usr/bin/env python3
"""Times the two steps of Tracking::TrackReferenceKeyFrame on 640x480 synthetic frames extracted with 500, 1 000 and 2 000 features:
  - the resident path, with HIP events on the stream both handles issue on, one frame (pair) and 32 frames (pairs) per call, medians of 30
    calls: amos_bow_transform_batch_device (two launches) and amos_match_bow_batch_device (two launches) on the FeatureVectors the
    transform left on the device.  The vocabulary is synthetic, k = 10 / L = 4 (11 111 nodes) with levelsup = 2, so the FeatureVector has
    about 100 nodes as ORBvoc's has at levelsup = 4; ORBvoc's two further levels of descent are NOT reproduced;
  - beside the search, for the same pair, the host class's SearchByBoW(pKF, F, ...) (ORBmatcherFor: one upload + list-distance kernel +
    download, the greedy loop on the host) and the C++ drop-in over the host form (amos_match_bow), both wall clock (std::chrono inside the
    harness, mean of 5 runs, median of 5 such means), NOT event-timed.  Both start with the stand-in objects built.
Prints one JSON line per feature count (medians in milliseconds)."""
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
    import bow_restatement as br
    import bow_search_cases as bc
    import host_bow_binding as hbb
    import oracle_binding as ob
    voc, levelsup = br.make_vocabulary(10, 4, seed=51, flips=80, bad_weight_share=0.02), 2
    side = torch.cuda.Stream()  # both handles issue on it, the events are recorded on it
    torch.cuda.set_stream(side)
    mt = pkg.OrbMatcher(stream=side.cuda_stream)
    bow = pkg.BowVocabulary(voc.k, voc.L, *voc.arrays(), stream=side.cuda_stream)

    def timed(call):
        times = []
        for rep in range(reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if rep >= 5:
                times.append(e0.elapsed_time(e1))
        return round(float(np.median(times)), 4)

    for nfeat in (500, 1000, 2000):
        orc = ob.Oracle(nfeat, 1.2, 8)
        frames = [orc.extract(synth.frame(3, k)) for k in range(2)]
        cap = max(len(k) for k, _ in frames) + 8
        out = {"features": [len(k) for k, _ in frames]}
        for nf in (1, 32):
            slots = 2 * nf  # slot 2 p: a keyframe, slot 2 p + 1: its frame
            kps, desc = np.zeros((slots, cap), pkg.KP_DTYPE), np.zeros((slots, cap, 32), np.uint8)
            counts = np.zeros(slots, np.int32)
            for s in range(slots):
                k, d = frames[s % 2]
                kps[s, :len(k)], desc[s, :len(k)], counts[s] = k, d, len(k)

            def up(a):
                return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
            d_kps, d_desc, d_counts = up(kps), up(desc), up(counts)
            i32 = dict(dtype=torch.int32, device="cuda")
            d_fw, d_fn, d_ids, d_idx, d_words = (torch.zeros((slots, cap), **i32) for _ in range(5))
            d_off, d_nn, d_nw = torch.zeros((slots, cap + 1), **i32), torch.zeros(slots, **i32), torch.zeros(slots, **i32)
            d_wts, d_bstats = torch.zeros((slots, cap), dtype=torch.float64, device="cuda"), torch.zeros((slots, 4), **i32)
            d_kf, d_f = up(np.arange(nf, dtype=np.int32) * 2), up(np.arange(nf, dtype=np.int32) * 2 + 1)
            d_match, d_stats = torch.zeros((nf, cap), **i32), torch.zeros((nf, 4), **i32)
            out[f"transform_ms_{slots}_frames"] = timed(lambda: bow.transform_batch_device(
                d_desc.data_ptr(), d_counts.data_ptr(), slots, cap, levelsup, d_fw.data_ptr(), d_fn.data_ptr(), d_nn.data_ptr(), d_ids.data_ptr(),
                d_off.data_ptr(), d_idx.data_ptr(), d_nw.data_ptr(), d_words.data_ptr(), d_wts.data_ptr(), d_bstats.data_ptr()))
            out[f"search_ms_{nf}_pairs"] = timed(lambda: mt.bow_batch_device(
                d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_nn.data_ptr(), d_ids.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(),
                d_kf.data_ptr(), d_f.data_ptr(), nf, cap, d_match.data_ptr(), d_stats.data_ptr(), nn_ratio=0.7, check_orientation=1))
            mt.sync()
            if nf == 1:
                st = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.BOW_SEARCH_STATS_DTYPE)[0]
                bs = np.frombuffer(d_bstats.cpu().numpy().tobytes(), pkg.BOW_STATS_DTYPE)[0]
                out.update(nodes=int(bs["n_nodes"]), words=int(bs["n_words"]), queries=int(st["n_queries"]), matches=int(st["n_matches"]),
                           researched_share=round(float(st["n_researched"]) / max(int(st["n_queries"]), 1), 4))
        sides = []
        for k, d in frames:  # the same FeatureVectors for the two host paths, from the host form of the transform
            t = bow.transform(d, levelsup)
            fv = {int(nid): t["node_idx"][t["node_off"][a]:t["node_off"][a + 1]].tolist() for a, nid in enumerate(t["node_ids"])}
            s = bc.side(d, k["angle"], fv)
            s["keys"] = np.ascontiguousarray(k, bc.KP)
            sides.append(s)
        for which in ("parent", "dropin"):
            ms = [hbb.search_by_bow(which, sides[0], sides[1], 0.7, 1, repeat=5)["ms"] for _ in range(5)]
            out[f"{which}_host_ms"] = round(float(np.median(ms)), 4)
        print(json.dumps(out), flush=True)
    bow.close()
    mt.close()


if __name__ == "__main__":
    main()
