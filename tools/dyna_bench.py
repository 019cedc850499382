"""Latency of the dynamic-object test on the device (amos_dyna_*, amos_orb_gate_labels_batch_device) with HIP events: the tail of
GetSceneFlowObj alone at n = 1000 tracked points; the CalDyna decision + labelled gate (+ describe) at 1 and 64 frames; and the whole chain
for one 640 x 480 frame pair (amos_dyna_scene_flow_obj_device + Lab + SLIC + k-means + decision + detect + labelled gate + describe),
eager and replayed from a graph.  Prints one JSON line.  Run it under `timeout`; for per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python tools/dyna_bench.py`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time(torch, stream, call, reps):
    for _ in range(3):
        call()
    stream.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record(stream)
        call()
        ev[1].record(stream)
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return round(float(np.median(times)), 1), round(float(np.min(times)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    import dyna_restatement as dr
    import test_gpu_dyna as tg
    pkg = entry.load_package()
    from amos_slam_amd import synth
    out = {"n": args.n, "reps": args.reps}
    s = torch.cuda.Stream()
    stream = torch.cuda.ExternalStream(s.cuda_stream)
    dyna = pkg.SceneFlowDyna(max_points=4096, max_frames=64, stream=s.cuda_stream)
    # ---- the tail alone
    rng = np.random.default_rng(3)
    sc = dr.scene(rng, args.n, moving=0.25)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(
        pre=sc["pre"], nxt=sc["nxt"], st=sc["state"], n=np.array([args.n], np.int32), F2=dr.fundamental_of(sc["T"]), fst=tg.F_OK,
        Rt=dr.rt_of(sc["T"]), pst=np.array([1, 1, 1, args.n, 1], np.int32), dl=sc["depth_last"], dc=sc["depth_cur"]).items()}
    cam, poses = tg._camera(pkg), pkg.DynaPoses.of(tg._perturbed(rng, sc["T"], 0.01))
    torch.cuda.synchronize()

    def tail(frame=0):
        dyna.tail_device(frame, d["pre"].data_ptr(), d["nxt"].data_ptr(), d["st"].data_ptr(), d["n"].data_ptr(), d["F2"].data_ptr(), d["fst"].data_ptr(),
                         d["Rt"].data_ptr(), d["pst"].data_ptr(), d["dl"].data_ptr(), 640, d["dc"].data_ptr(), 640, 640, 480, cam, dr.FX, dr.FY, poses)
    out["tail_us_median"], out["tail_us_min"] = _time(torch, stream, tail, args.reps)
    for f in range(64):
        tail(f)
    # ---- decision + labelled gate + describe at 1 and 64 frames (SLIC / k-means labels)
    d_labels, d_centers, nc = tg._slic_labels(pkg, synth, 64)
    frames = synth.frames(3, 4, 64)
    masks = np.stack([synth.person_mask(3, 4 + k) for k in range(64)])
    d_frames, d_masks = torch.from_numpy(frames).cuda(), torch.from_numpy(masks).cuda()
    d_rm = torch.zeros((64, 15), dtype=torch.int32, device="cuda")
    d_gst = torch.zeros(64, dtype=torch.int32, device="cuda")
    for nb in (1, 64):
        ext = pkg.OrbExtractor(max_batch=nb, stream=s.cuda_stream)
        torch.cuda.synchronize()

        def decide():
            dyna.decide_batch_device(nb, d_labels.data_ptr(), 480 * 640, 640, 640, 480, d_centers.data_ptr(), nc, nc, 15, d_rm.data_ptr(), 15)

        def gate():
            ext.gate_labels_batch_device(d_masks.data_ptr(), 480 * 640, 640, d_labels.data_ptr(), 480 * 640, 640, d_centers.data_ptr(), nc, nc,
                                         d_rm.data_ptr(), 15, 15, d_gst.data_ptr())
        ext.detect_batch_device(d_frames.data_ptr(), 480 * 640, 640, 640, 480, nb)
        out[f"decide_batch{nb}_us_median"], out[f"decide_batch{nb}_us_min"] = _time(torch, stream, decide, args.reps)
        out[f"gate_labels_batch{nb}_us_median"], _ = _time(torch, stream, gate, args.reps)

        def decide_gate_describe():
            decide()
            ext.detect_batch_device(d_frames.data_ptr(), 480 * 640, 640, 640, 480, nb)
            gate()
            ext.describe_batch_device()

        def detect_describe():
            ext.detect_batch_device(d_frames.data_ptr(), 480 * 640, 640, 640, 480, nb)
            ext.describe_batch_device()
        full, _ = _time(torch, stream, decide_gate_describe, max(5, args.reps // 5))
        base, _ = _time(torch, stream, detect_describe, max(5, args.reps // 5))
        out[f"decide_gate_batch{nb}_over_detect_describe_us"] = round(full - base, 1)
        del ext
    # ---- the whole chain for one frame pair, eager and from a graph
    ch = tg._Chain(pkg, synth, s.cuda_stream)
    out["chain_eager_us_median"], out["chain_eager_us_min"] = _time(torch, stream, ch.run, max(5, args.reps // 5))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ch.run()

    def replay():
        with torch.cuda.stream(s):
            g.replay()
    out["chain_graph_us_median"], out["chain_graph_us_min"] = _time(torch, stream, replay, max(5, args.reps // 5))
    r = ch.outputs()
    out["chain_counts"] = [int(v) for v in r[0]["counts"]]
    out["chain_removed_clusters"] = int(r[1].sum())
    dyna.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
