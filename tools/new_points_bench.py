#!/usr/bin/env python3
"""Times LocalMapping::CreateNewMapPoints up to its `new MapPoint` on 640x480 synthetic keyframes extracted with 500, 1 000 and 2 000
features (the FeatureVectors of tools/triangulation_bench.py: the synthetic k = 10 / L = 4 vocabulary at levelsup = 2), one keyframe
against 1, 10 and 20 neighbours; 30 % of the features hold a map point, 40 % are stereo with depths from u_right; camera k stands where
the stream's image shift puts it for a scene at depth 1.  Each point is the median of 30 calls after 5 warm-up calls:
  - device_ms: amos_match_triangulation_batch_device + amos_match_new_points_batch_device on resident frames (four launches), HIP
    events on the matcher's stream around the Python calls; device_new_points_ms: the second entry alone (two launches) on the rows the first left;
  - host_form_ms: amos_match_new_points (ONE call for all neighbours) through OrbMatcher.new_points, wall clock (the wrapper builds the
    views inside);
  - dropin_ms: ORB_SLAM2::CreateNewMapPointCandidates (KeyFrameNewPoints.h) on stand-in objects, wall clock (std::chrono in the harness);
  - parent_ms: what the mapping thread ran before on the same objects, same run: the drop-in search for all neighbours, then the
    host-compiled core looped over neighbours and matches.
Prints one JSON line per feature count (milliseconds)."""
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
    import host_new_points_binding as hnb
    import kf_search_cases as kc
    import new_points_cases as nc
    import new_points_restatement as nr
    import oracle_binding as ob
    voc, levelsup = br.make_vocabulary(10, 4, seed=51, flips=80, bad_weight_share=0.02), 2
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    mt = pkg.OrbMatcher(stream=side.cuda_stream)
    bow = pkg.BowVocabulary(voc.k, voc.L, *voc.arrays(), stream=side.cuda_stream)
    w, h, n_neigh = 640, 480, 20
    K, (sf, sg) = kc.camera(w, h), kc.levels(8)
    Kt = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    mbf = 0.08 * K[0, 0]
    step = np.array([2.0 / K[0, 0], 1.0 / K[1, 1], 0.0])
    cams = [nr.camera(np.eye(3), -k * step, Kt, 0.001, mbf, 1.2) for k in range(n_neigh + 1)]
    geos = [pkg.kf_geometry_from_poses(cams[0], cams[k]) for k in range(1, n_neigh + 1)]
    assert all(ok for _, ok in geos)
    geos = np.stack([g for g, _ in geos])

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
            s = bc.side(desc, kps["angle"], fv, (rng.random(len(kps)) < 0.3).astype(np.uint8))
            s["keys"] = np.ascontiguousarray(kps, bc.KP)
            s["u_right"] = np.where(rng.random(len(kps)) < 0.4, kps["x"] - rng.uniform(3, 30, len(kps)), -1.0).astype(np.float32)
            sides.append(nc.with_depth(s, mbf))
        cap = max(len(s["desc"]) for s in sides) + 8
        out = {"features": len(sides[0]["desc"]), "nodes": len(sides[0]["fv"])}
        a = kc.pack(sides, cap)
        d = {k: up(v) for k, v in a.items()}
        depth = np.zeros((len(sides), cap), np.float32)
        for k, s in enumerate(sides):
            depth[k, :len(s["depth"])] = s["depth"]
        d_depth, d_sf, d_sg = up(depth), up(sf), up(sg)
        for n2 in (1, 10, 20):
            pairs = np.array([(0, k) for k in range(1, n2 + 1)], np.int32)
            d_1, d_2 = up(pairs[:, 0]), up(pairs[:, 1])
            d_match = torch.zeros((n2, cap), dtype=torch.int32, device="cuda")
            d_sstats = torch.zeros((n2, 4), dtype=torch.int32, device="cuda")
            d_new = torch.zeros((n2, cap, 6), dtype=torch.int32, device="cuda")
            d_stats = torch.zeros((n2, 16), dtype=torch.int32, device="cuda")
            d_geo = up(geos[:n2])

            def search():
                mt.triangulation_batch_device(d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d["n_nodes"].data_ptr(),
                                              d["node_ids"].data_ptr(), d["node_off"].data_ptr(), d["node_idx"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(),
                                              n2, cap, d_geo.data_ptr(), d_sf.data_ptr(), d_sg.data_ptr(), len(sf), d_match.data_ptr(), d_sstats.data_ptr(),
                                              only_stereo=False, check_orientation=False, d_has_point=d["has_point"].data_ptr(),
                                              d_u_right=d["u_right"].data_ptr())

            def new_points():
                mt.new_points_batch_device(d["kps"].data_ptr(), d["counts"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(), pairs, cap, d_match.data_ptr(),
                                           d_sf.data_ptr(), d_sg.data_ptr(), len(sf), np.stack(cams), d_new.data_ptr(), d_stats.data_ptr(),
                                           d_u_right=d["u_right"].data_ptr(), d_depth=d_depth.data_ptr())

            def both():
                search()
                new_points()
            r = {"device_ms": events(both), "device_new_points_ms": events(new_points)}
            mt.sync()
            st = np.frombuffer(d_stats.cpu().numpy().tobytes(), pkg.NEW_POINTS_STATS_DTYPE)
            r.update(matches=int(st["n_matches"].sum()), new=int(st["n_new"].sum()), claimed=int(st["n_verdict"][:, pkg.NEW_POINT_CLAIMED].sum()))
            k1, k2s = kc.with_csr(sides[0]), [kc.with_csr(s) for s in sides[1:n2 + 1]]
            r["host_form_ms"] = wall(lambda: mt.new_points(k1, k2s, cams[0], np.stack(cams[1:n2 + 1]), sf, sg))
            _, stats = mt.new_points(k1, k2s, cams[0], np.stack(cams[1:n2 + 1]), sf, sg)
            assert int(stats["n_new"].sum()) == r["new"]
            case = {"sides": sides[:n2 + 1], "cams": cams[:n2 + 1], "levels": (sf, sg)}
            for which in ("dropin", "parent"):
                ret, rows, _, ms = hnb.dropin(which, case, repeat=reps + warm)
                r[f"{which}_ms"] = med(ms)
                assert ret == r["new"], which
            out[f"new_points_{n2}"] = r
        print(json.dumps(out), flush=True)
    bow.close()
    mt.close()


if __name__ == "__main__":
    main()
