#!/usr/bin/env python3
"""Times the mapping thread's two keyframe pair searches on 640x480 synthetic keyframes extracted with 500, 1 000 and 2 000 features, with
the FeatureVectors of the synthetic k = 10 / L = 4 vocabulary at levelsup = 2 (about 100 nodes, as tools/bow_bench.py):
  - SearchForTriangulation, one keyframe against 1, 10 and 20 neighbours (LocalMapping::CreateNewMapPoints); 30 % of the features hold a map
    point, 40 % are stereo, F12 follows the stream's image shift;
  - SearchByBoW(KF, KF), one keyframe against 1 and 8 candidates (LoopClosing::ComputeSim3); 80 % of the features hold a map point.
Each point is the median of 30 calls after 5 warm-up calls:
  - device_ms: the two launches of the batch form on resident frames, HIP events on the matcher's stream;
  - host_form_ms: amos_match_triangulation (ONE call for all neighbours) / amos_match_bow_kf (one call per candidate), wall clock around
    the C call with the views built;
  - dropin_ms: the C++ drop-in of KeyFrameSearch.h on stand-in objects, wall clock (std::chrono inside the harness);
  - parent_ms: the host class ORBmatcherFor looped over the neighbours on the same objects, wall clock alike: what the mapping thread ran
    before.
Prints one JSON line per feature count (milliseconds)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(reps=30, warm=5):
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import importlib
    synth = importlib.import_module("amos_slam_amd.synth")
    import bow_restatement as br
    import bow_search_cases as bc
    import host_kf_binding as hk
    import kf_search_cases as kc
    import oracle_binding as ob
    voc, levelsup = br.make_vocabulary(10, 4, seed=51, flips=80, bad_weight_share=0.02), 2
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    mt = pkg.OrbMatcher(stream=side.cuda_stream)
    bow = pkg.BowVocabulary(voc.k, voc.L, *voc.arrays(), stream=side.cuda_stream)
    w, h, n_neigh = 640, 480, 20
    K, (R12, t12) = kc.camera(w, h), kc.shift_motions(w, h)["general"]
    geo, (sf, sg) = kc.geometry(K, R12, t12), kc.levels(8)
    pose = hk.pose_of_neighbour(R12, t12)
    L = pkg.lib()

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    def events(call):
        times = []
        for rep in range(reps + warm):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if rep >= warm:
                times.append(e0.elapsed_time(e1))
        return round(float(np.median(times)), 4)

    def wall(call):
        times = []
        for rep in range(reps + warm):
            t0 = time.perf_counter()
            call()
            if rep >= warm:
                times.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(times)), 4)

    def med(ms):
        return round(float(np.median(ms[warm:])), 4)

    for nfeat in (500, 1000, 2000):
        orc = ob.Oracle(nfeat, 1.2, 8)
        rng = np.random.default_rng(nfeat)
        sides = []
        for k in range(n_neigh + 1):  # keyframe 0 and its neighbours: the scene moved by (2 k, k) pixels
            kps, desc = orc.extract(synth.frame(3, k))
            t = bow.transform(desc, levelsup)
            fv = {int(nid): t["node_idx"][t["node_off"][a]:t["node_off"][a + 1]].tolist() for a, nid in enumerate(t["node_ids"])}
            s = bc.side(desc, kps["angle"], fv)
            s["keys"] = np.ascontiguousarray(kps, bc.KP)
            s["u_right"] = np.where(rng.random(len(kps)) < 0.4, kps["x"] - rng.uniform(3, 30, len(kps)), -1.0).astype(np.float32)
            s["draw"] = rng.random(len(kps))
            sides.append(s)
        cap = max(len(s["desc"]) for s in sides) + 8
        out = {"features": len(sides[0]["desc"]), "nodes": len(sides[0]["fv"])}

        def resident(share):
            a = kc.pack([dict(s, has_point=(s["draw"] < share).astype(np.uint8)) for s in sides], cap)
            return {k: up(v) for k, v in a.items()}

        def batch_args(d, n2):
            d_1, d_2 = up(np.zeros(n2, np.int32)), up(np.arange(1, n2 + 1, dtype=np.int32))
            d_match = torch.zeros((n2, cap), dtype=torch.int32, device="cuda")
            d_stats = torch.zeros((n2, 4), dtype=torch.int32, device="cuda")
            common = (d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d["n_nodes"].data_ptr(), d["node_ids"].data_ptr(),
                      d["node_off"].data_ptr(), d["node_idx"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(), n2, cap)
            return common, d_match, d_stats, (d_1, d_2)

        # ---- SearchForTriangulation
        d = resident(0.3)
        tri_sides = [dict(s, has_point=(s["draw"] < 0.3).astype(np.uint8)) for s in sides]
        d_sf, d_sg = up(sf), up(sg)
        for n2 in (1, 10, 20):
            common, d_match, d_stats, keep = batch_args(d, n2)
            d_geo = up(np.stack([geo] * n2))
            r = {"device_ms": events(lambda: mt.triangulation_batch_device(
                *common, d_geo.data_ptr(), d_sf.data_ptr(), d_sg.data_ptr(), len(sf), d_match.data_ptr(), d_stats.data_ptr(), only_stereo=False,
                check_orientation=False, d_has_point=d["has_point"].data_ptr(), d_u_right=d["u_right"].data_ptr()))}
            mt.sync()
            st = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.BOW_SEARCH_STATS_DTYPE)
            r.update(matches=int(st["n_matches"].sum()), researched=int(st["n_researched"].sum()), queries=int(st["n_queries"].sum()))
            views = [pkg.OrbMatcher._bow_view(*[kc.with_csr(s)[k] for k in ("keys", "desc", "node_ids", "node_off", "node_idx", "has_point", "u_right")])
                     for s in tri_sides[:n2 + 1]]
            ptrs = (C.c_void_p * n2)(*[C.addressof(v) for v, _ in views[1:]])
            geos, m12, stats = np.stack([geo] * n2), np.zeros((n2, views[0][0].n), np.int32), np.zeros(n2, pkg.BOW_SEARCH_STATS_DTYPE)
            r["host_form_ms"] = wall(lambda: L.amos_match_triangulation(mt.h, C.byref(views[0][0]), ptrs, n2, pkg._p(geos), pkg._p(sf), pkg._p(sg),
                                                                        len(sf), 0, 0, pkg._p(m12), pkg._p(stats)))
            assert int(stats["n_matches"].sum()) == r["matches"]
            for which in ("dropin", "parent"):
                res = hk.triangulation(which, tri_sides[0], tri_sides[1:n2 + 1], K, [pose] * n2, [geo["f12"]] * n2, sf, 0, 0, repeat=reps + warm)
                r[f"{which}_ms"] = med(res["ms"])
                assert sum(len(p) for p in res["pairs"]) == r["matches"], which
            out[f"triangulation_{n2}"] = r
        # ---- SearchByBoW(KF, KF)
        d = resident(0.8)
        bow_sides = [dict(s, has_point=(s["draw"] < 0.8).astype(np.uint8)) for s in sides]
        for n2 in (1, 8):
            common, d_match, d_stats, keep = batch_args(d, n2)
            r = {"device_ms": events(lambda: mt.bow_kf_batch_device(*common, d_match.data_ptr(), d_stats.data_ptr(), nn_ratio=0.75,
                                                                    check_orientation=True, d_has_point=d["has_point"].data_ptr()))}
            mt.sync()
            st = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.BOW_SEARCH_STATS_DTYPE)
            r.update(matches=int(st["n_matches"].sum()), researched=int(st["n_researched"].sum()), queries=int(st["n_queries"].sum()))
            views = [pkg.OrbMatcher._bow_view(*[kc.with_csr(s)[k] for k in ("keys", "desc", "node_ids", "node_off", "node_idx", "has_point")])
                     for s in bow_sides[:n2 + 1]]
            m12, stats = np.zeros(views[0][0].n, np.int32), np.zeros(1, pkg.BOW_SEARCH_STATS_DTYPE)

            def host_form():
                for v, _ in views[1:]:
                    L.amos_match_bow_kf(mt.h, C.byref(views[0][0]), C.byref(v), 0.75, 1, pkg._p(m12), pkg._p(stats))
            r["host_form_ms"] = wall(host_form)
            for which in ("dropin", "parent"):
                res = hk.search_by_bow(which, bow_sides[0], bow_sides[1:n2 + 1], 0.75, 1, repeat=reps + warm)
                r[f"{which}_ms"] = med(res["ms"])
                assert int(res["returned"].sum()) == r["matches"], which
            out[f"bow_kf_{n2}"] = r
        print(json.dumps(out), flush=True)
    bow.close()
    mt.close()


if __name__ == "__main__":
    main()
