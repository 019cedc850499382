"""GPU: amos_dyna_* (the tail of Tracking::GetSceneFlowObj and CalDyna's moving-cluster decision on the device) and
amos_orb_gate_labels_batch_device against tests/dyna_restatement.py, the host gate and the oracle, bit for bit; the whole chain
GetSceneFlowObj -> cluster -> decision -> labelled gate -> describe eagerly and replayed from a graph."""
import os
import sys

import numpy as np
import pytest

import dyna_restatement as dr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
MAXP = 4096
F_OK = np.array([1, 50, 10, 100, 1, 40, 10, 90], np.int32)
KEYS = ("counts", "pose", "rwc", "ow", "match", "rpe", "epipolar", "tm", "flow")


@pytest.fixture(scope="module")
def dyna(gpu_lib):
    h = gpu_lib.SceneFlowDyna(max_points=MAXP, max_frames=64)
    yield h
    h.close()


def _camera(gpu_lib, Tlw=None):
    cam = gpu_lib.SceneFlowCamera(*(float(c) for c in dr.CAM))
    for i, v in enumerate((np.eye(3, 4, dtype=np.float32) if Tlw is None else np.asarray(Tlw, np.float32)).reshape(-1)):
        cam.Tlw[i] = float(v)
    return cam


def _same(got, want, what):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, a[:4], b[:4])
    assert got["choice"] == want["choice"] and got["status"] == want["status"], (what, got["choice"], want["choice"], got["status"], want["status"])


def _tail_case(gpu_lib, dyna, frame, sc, n, F2, fst, Rt, pst, motion, lk=None):
    import torch
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(
        pre=sc["pre"], nxt=sc["nxt"], st=sc["state"], n=np.array([n], np.int32), F2=np.asarray(F2, np.float64), fst=np.asarray(fst, np.int32),
        Rt=np.asarray(Rt, np.float64), pst=np.asarray(pst, np.int32), dl=sc["depth_last"], dc=sc["depth_cur"]).items()}
    torch.cuda.synchronize()
    poses = gpu_lib.DynaPoses.of(motion, lk)
    dyna.tail_device(frame, d["pre"].data_ptr(), d["nxt"].data_ptr(), d["st"].data_ptr(), d["n"].data_ptr(), d["F2"].data_ptr(), d["fst"].data_ptr(),
                     d["Rt"].data_ptr(), d["pst"].data_ptr(), d["dl"].data_ptr(), 640, d["dc"].data_ptr(), 640, 640, 480,
                     _camera(gpu_lib, sc["Tlw"]), dr.FX, dr.FY, poses)
    got = dyna.fetch(frame, n_tracked=n if 0 <= n <= MAXP else 0)
    want = dr.tail(sc["pre"], sc["nxt"], sc["state"], n, F2, fst, Rt, pst, sc["depth_last"], sc["depth_cur"], dr.CAM, sc["Tlw"], dr.FX, dr.FY,
                   motion, lk, max_points=MAXP)
    return got, want


def _perturbed(rng, T, s):
    P = np.asarray(T, np.float32).copy()
    P[:, 3] += rng.normal(0, s, 3).astype(np.float32)
    return P


# (seed, n, what): what picks the poses / models
TAIL_CASES = [(0, 0, "pnp"), (1, 1, "pnp"), (2, 7, "mm"), (3, 1000, "pnp"), (4, 1000, "mm"), (5, 1000, "lk"), (6, 1000, "no_pnp"),
              (7, 1000, "no_f2"), (8, MAXP, "pnp"), (9, MAXP, "mm"), (10, 1000, "tlw"), (11, 1000, "tie")]


@pytest.mark.parametrize("seed,n,what", TAIL_CASES)
def test_tail_equals_the_restatement(gpu_lib, dyna, seed, n, what):
    rng = np.random.default_rng(100 + seed)
    sc = dr.scene(rng, max(n, 1), moving=0.25, Tlw=dr.small_pose(rng) if what == "tlw" else None)
    T = sc["T"]
    F2, fst, pst = dr.fundamental_of(T), F_OK, np.array([1, 500, 40, n, 1], np.int32)
    good, bad = T, _perturbed(rng, T, 0.01)
    Rt, motion, lk = dr.rt_of(good), bad, None
    if what == "mm":
        Rt, motion = dr.rt_of(bad), good
    elif what == "lk":
        Rt, motion, lk = dr.rt_of(good), _perturbed(rng, T, 0.002), bad
    elif what == "no_pnp":
        Rt, pst, motion = np.zeros(12), np.array([0, 0, 500, n, 0], np.int32), good
    elif what == "no_f2":
        F2, fst = np.zeros(9), np.array([1, 50, 10, 100, 0, 0, 10, 90], np.int32)
    elif what == "tie":
        motion = T
    got, want = _tail_case(gpu_lib, dyna, seed % 64, sc, n, F2, fst, Rt, pst, motion, lk)
    _same(got, want, (seed, n, what))
    if n >= 1000:
        assert want["counts"][1] > 0.5 * n and want["counts"][4] > 0 and want["counts"][5] > 0
        assert want["choice"] == {"pnp": 1, "mm": 0, "no_pnp": 0, "tie": 1}.get(what, want["choice"])
    if what == "tie":
        assert want["counts"][2] == want["counts"][3]


def test_tail_rejects_a_count_out_of_range_and_resets(gpu_lib, dyna):
    rng = np.random.default_rng(7)
    sc = dr.scene(rng, 10)
    got, want = _tail_case(gpu_lib, dyna, 3, sc, MAXP + 1, np.zeros(9), F_OK, np.zeros(12), [1, 0, 0, 0, 0], np.eye(3, 4, dtype=np.float32))
    assert got["status"] == want["status"] == dr.BAD_N and np.all(got["counts"] == 0)
    dyna.reset_frame_device(3)
    r = dyna.fetch(3)
    assert r["status"] == dr.RESET and np.all(r["counts"] == 0)


def test_tail_rejects_an_infinite_focal_length(gpu_lib, dyna):
    """the PnP entry points' camera rule (finite, positive fx / fy) holds for the tail alone too; every buffer is real and n = 0"""
    import torch
    z = torch.zeros(640 * 480, dtype=torch.float32, device="cuda")
    args = lambda fx, fy: (0, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                           z.data_ptr(), 640, z.data_ptr(), 640, 640, 480, _camera(gpu_lib), fx, fy, gpu_lib.DynaPoses.of(np.eye(3, 4, dtype=np.float32)))
    for fx, fy in ((float("inf"), dr.FY), (dr.FX, float("inf"))):
        with pytest.raises(gpu_lib.AmosError):
            dyna.tail_device(*args(fx, fy))
    dyna.tail_device(*args(dr.FX, dr.FY))
    assert np.all(dyna.fetch(0)["counts"] == 0)


def _tails(gpu_lib, dyna, n_frames, n=400):
    """slot f: a tail on a scene of seed f (moving points), returns the fetched lists"""
    out = []
    for f in range(n_frames):
        rng = np.random.default_rng(500 + f)
        sc = dr.scene(rng, n, moving=0.3)
        got, _ = _tail_case(gpu_lib, dyna, f, sc, n, dr.fundamental_of(sc["T"]), F_OK, dr.rt_of(sc["T"]), [1, 1, 1, n, 1],
                            _perturbed(rng, sc["T"], 0.01))
        out.append(got)
    return out


def _slic_labels(gpu_lib, synth, n_frames, k=15, seed=1):
    """labels and centres (ids from the k-means) of synthetic frames from amos_slic_batch_device + amos_cluster_kmeans_batch_device"""
    import torch
    gray = synth.frames(5, 0, n_frames)
    lab = np.repeat(gray[..., None], 3, axis=3)
    yy, xx = np.mgrid[0:480, 0:640]
    depth = np.broadcast_to((8000 + 3000 * np.sin(xx / 100.0)).astype(np.uint16), (n_frames, 480, 640)).copy()
    s = gpu_lib.Slic(max_batch=n_frames)
    nc = s.center_count(640, 480)[0]
    d_lab, d_depth = torch.from_numpy(lab).cuda(), torch.from_numpy(depth).cuda()
    d_labels = torch.zeros((n_frames, 480, 640), dtype=torch.float64, device="cuda")
    d_centers = torch.zeros((n_frames, nc, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s.run_batch_device(d_lab.data_ptr(), d_depth.data_ptr(), 640, 480, n_frames, d_labels.data_ptr(), d_centers.data_ptr())
    s.kmeans_batch_device(d_centers.data_ptr(), nc, n_frames, k=k, seed=seed)
    s.sync()
    s.close()
    return d_labels, d_centers, nc


def _hand_labels(n_frames, rng):
    import torch
    labels = np.stack([np.kron(rng.integers(0, 49, (15, 20)), np.ones((32, 32))) for _ in range(n_frames)]).astype(np.float64)  # 0 = none
    centers = np.zeros((n_frames, 48, 8), np.int32)
    centers[..., 6] = np.arange(1, 49)
    centers[..., 7] = rng.integers(0, 15, (n_frames, 48))
    if n_frames > 1:
        centers[1, 5, 7] = 40  # an id outside [0, k)
    return torch.from_numpy(labels).cuda(), torch.from_numpy(centers).cuda(), 48


def _decide_and_check(gpu_lib, dyna, tails, d_labels, d_centers, nc, k=15):
    import torch
    nf = len(tails)
    d_rm = torch.full((nf, 16), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dyna.decide_batch_device(nf, d_labels.data_ptr(), 480 * 640, 640, 640, 480, d_centers.data_ptr(), nc, nc, k, d_rm.data_ptr(), 16)
    torch.cuda.ExternalStream(dyna.stream).synchronize()
    rm = d_rm.cpu().numpy()
    labels, centers = d_labels.cpu().numpy(), d_centers.cpu().numpy()
    removed = 0
    for f in range(nf):
        g = dyna.fetch(f, k=k)
        wrm, wave, wep, wst = dr.decide(tails[f]["match"], tails[f]["rpe"], tails[f]["tm"], labels[f], centers[f, :, 7], k)
        assert rm[f, :k].tobytes() == wrm.tobytes() and np.all(rm[f, k:] == 7), (f, rm[f], wrm)
        assert g["ave_rpe"].tobytes() == wave.tobytes() and g["ep_num"].tobytes() == wep.tobytes() and g["decide_status"] == wst, f
        removed += int(wrm.sum())
    return removed


@pytest.mark.parametrize("n_frames", [1, 8, 64])
def test_decision_on_slic_kmeans_labels(gpu_lib, dyna, synth, n_frames):
    tails = _tails(gpu_lib, dyna, n_frames)
    d_labels, d_centers, nc = _slic_labels(gpu_lib, synth, n_frames)
    _decide_and_check(gpu_lib, dyna, tails, d_labels, d_centers, nc)


@pytest.mark.parametrize("n_frames", [1, 8, 64])
def test_decision_on_hand_made_labels_with_zeros(gpu_lib, dyna, n_frames):
    tails = _tails(gpu_lib, dyna, n_frames, n=300)
    d_labels, d_centers, nc = _hand_labels(n_frames, np.random.default_rng(n_frames))
    assert _decide_and_check(gpu_lib, dyna, tails, d_labels, d_centers, nc) > 0


def test_labelled_batch_gate_equals_host_gate_and_oracle(gpu_lib, ob, synth):
    import torch
    n = 4
    frames = synth.frames(3, 4, n)
    masks = np.stack([synth.person_mask(3, 4 + k) for k in range(n)])
    masks[2] = 0
    rng = np.random.default_rng(11)
    labels = np.stack([np.kron(rng.integers(1, 49, (15, 20)), np.ones((32, 32))) for _ in range(n)]).astype(np.float64)
    centers = np.zeros((n, 48, 8), np.int32)
    centers[..., 6] = np.arange(1, 49)
    centers[..., 7] = rng.integers(0, 15, (n, 48))
    rm = np.zeros((n, 15), np.int32)
    for f in range(n):
        rm[f, rng.choice(15, 3 + f, replace=False)] = 1
    ext = gpu_lib.OrbExtractor(max_batch=n)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(fr=frames, m=masks, l=labels, c=centers, rm=rm).items()}
    d_status = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.detect_batch_device(d["fr"].data_ptr(), 480 * 640, 640, 640, 480, n)
    ext.gate_labels_batch_device(d["m"].data_ptr(), 480 * 640, 640, d["l"].data_ptr(), 480 * 640, 640, d["c"].data_ptr(), 48, 48, d["rm"].data_ptr(),
                                 15, 15, d_status.data_ptr())
    ext.describe_batch_device()
    ext.sync()
    assert np.all(d_status.cpu().numpy() == 0)
    host = gpu_lib.OrbExtractor()
    for f in range(n):
        orc = ob.Oracle()
        orc.detect(frames[f])
        orc.gate(masks[f], labels[f], centers[f, :, 7].copy(), rm[f])
        ko, do = orc.describe()
        host.detect(frames[f])
        host.gate(masks[f], labels[f], centers[f, :, 7].copy(), rm[f])
        kh, dh = host.describe()
        kg, dg = ext.batch_fetch(f)
        assert kg.tobytes() == ko.tobytes() and dg.tobytes() == do.tobytes(), f
        assert kg.tobytes() == kh.tobytes() and dg.tobytes() == dh.tobytes(), f
    labelled = sum(len(ext.batch_fetch(f)[0]) for f in range(n))
    ext.detect_batch_device(d["fr"].data_ptr(), 480 * 640, 640, 640, 480, n)  # the mask alone keeps more
    ext.gate_batch_device(d["m"].data_ptr(), 480 * 640, 640)
    ext.describe_batch_device()
    ext.sync()
    assert sum(len(ext.batch_fetch(f)[0]) for f in range(n)) > labelled


def _moving_pair(synth):
    """frame k + 1 of a synthetic stream is frame k shifted by (2, 1) px; a textured block moves by (14, 9) px and sits nearer"""
    f0, f1 = synth.frame(9, 10).copy(), synth.frame(9, 11).copy()
    rng = np.random.default_rng(77)
    block = (rng.integers(0, 2, (12, 12)) * 200 + 30).astype(np.uint8)
    block = np.kron(block, np.ones((8, 8), np.uint8))
    f0[180:276, 300:396] = block
    f1[189:285, 314:410] = block
    depth0 = np.full((480, 640), 2.0, np.float32)
    depth1 = depth0.copy()
    depth0[180:276, 300:396] = 1.0
    depth1[189:285, 314:410] = 1.0
    depth0[:30] = 0
    return f0, f1, depth0, depth1


class _Chain:
    """GetSceneFlowObj -> Lab -> SLIC -> k-means -> decide -> detect -> labelled gate -> describe on one stream"""

    def __init__(self, gpu_lib, synth, stream):
        import torch
        self.f0, self.f1, self.z0, self.z1 = _moving_pair(synth)
        self.corners = gpu_lib.CornerDetector(stream=stream)
        self.lk = gpu_lib.LkTracker(640, 480, stream=stream)
        self.fmat = gpu_lib.FundamentalRansac(max_points=1000, max_problems=1, stream=stream)
        self.pnp = gpu_lib.PnpRansac(max_points=1000, max_problems=1, stream=stream)
        self.dyna = gpu_lib.SceneFlowDyna(max_points=1000, max_frames=1, stream=stream)
        self.slic = gpu_lib.Slic(max_batch=1, stream=stream)
        self.ext = gpu_lib.OrbExtractor(max_batch=1, stream=stream)
        self.nc = self.slic.center_count(640, 480)[0]
        bgr = np.repeat(self.f1[..., None], 3, axis=2)
        depth16 = (self.z1 * 5000).astype(np.uint16)
        self.d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(
            g0=self.f0, g1=self.f1, z0=self.z0, z1=self.z1, bgr=bgr, d16=depth16, mask=np.zeros((480, 640), np.uint8)).items()}
        self.d["lab"] = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda")
        self.d["labels"] = torch.zeros((480, 640), dtype=torch.float64, device="cuda")
        self.d["centers"] = torch.zeros((self.nc, 8), dtype=torch.int32, device="cuda")
        self.d["rm"] = torch.zeros(15, dtype=torch.int32, device="cuda")
        self.d["gst"] = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.cam = _camera(gpu_lib)
        self.poses = gpu_lib.DynaPoses.of(np.eye(3, 4, dtype=np.float32))
        torch.cuda.synchronize()

    def run(self):
        d = self.d
        self.dyna.scene_flow_obj_device(0, self.corners, self.lk, self.fmat, self.pnp, d["g0"].data_ptr(), 640, d["g1"].data_ptr(), 640, 640, 480,
                                        d["z0"].data_ptr(), 640, d["z1"].data_ptr(), 640, self.cam, dr.FX, dr.FY, self.poses)
        self.slic.bgr2lab_batch_device(d["bgr"].data_ptr(), 480 * 640, d["lab"].data_ptr())
        self.slic.run_batch_device(d["lab"].data_ptr(), d["d16"].data_ptr(), 640, 480, 1, d["labels"].data_ptr(), d["centers"].data_ptr())
        self.slic.kmeans_batch_device(d["centers"].data_ptr(), self.nc, 1, k=15, seed=1)
        self.dyna.decide_batch_device(1, d["labels"].data_ptr(), 480 * 640, 640, 640, 480, d["centers"].data_ptr(), self.nc, self.nc, 15,
                                      d["rm"].data_ptr(), 15)
        self.ext.detect_batch_device(d["g1"].data_ptr(), 480 * 640, 640, 640, 480, 1)
        self.ext.gate_labels_batch_device(d["mask"].data_ptr(), 480 * 640, 640, d["labels"].data_ptr(), 480 * 640, 640, d["centers"].data_ptr(),
                                          self.nc, self.nc, d["rm"].data_ptr(), 15, 15, d["gst"].data_ptr())
        self.ext.describe_batch_device()

    def outputs(self):
        import torch
        torch.cuda.ExternalStream(self.dyna.stream).synchronize()
        r = self.dyna.fetch(0, n_tracked=1000, k=15)
        kps, desc = self.ext.batch_fetch(0)
        return r, self.d["rm"].cpu().numpy(), kps, desc, self.d["labels"].cpu().numpy(), self.d["centers"].cpu().numpy()


def _chain_want(gpu_lib, ob, ch, res):
    """the same steps composed from the existing entries (separate handles) and the restatement"""
    import torch
    import flow_oracle as fo
    det = gpu_lib.CornerDetector()
    lk = gpu_lib.LkTracker(640, 480, stream=det.stream)
    fmat = gpu_lib.FundamentalRansac(max_points=1000, max_problems=1, stream=det.stream)
    pnp = gpu_lib.PnpRansac(max_points=1000, max_problems=1, stream=det.stream)
    st = torch.cuda.ExternalStream(det.stream)
    d0, d1 = ch.d["g0"], ch.d["g1"]
    d_xy = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.good_features_device(d0.data_ptr(), 640, 640, 480, d_xy.data_ptr(), 1000, d_n.data_ptr())
    det.subpix_device(d0.data_ptr(), 640, 640, 480, d_xy.data_ptr(), count_ptr=d_n.data_ptr(), n=1000)
    st.synchronize()
    n = int(d_n.item())
    d_next = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    d_lk = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_state = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lk.track_device(d0.data_ptr(), 640, d1.data_ptr(), 640, d_xy.data_ptr(), n, d_next.data_ptr(), d_lk.data_ptr())
    gpu_lib.flow_check(det.stream, d0.data_ptr(), 640, d1.data_ptr(), 640, 640, 480, d_xy.data_ptr(), d_next.data_ptr(), d_lk.data_ptr(), n,
                       d_state.data_ptr())
    F1, F2 = (torch.zeros(9, dtype=torch.float64, device="cuda") for _ in range(2))
    keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
    fst = torch.zeros(8, dtype=torch.int32, device="cuda")
    fmat.scene_flow_pair_device(d_xy.data_ptr(), d_next.data_ptr(), d_state.data_ptr(), d_n.data_ptr(), F1.data_ptr(), F2.data_ptr(), keep.data_ptr(),
                                fst.data_ptr())
    Rt = torch.zeros(12, dtype=torch.float64, device="cuda")
    pst = torch.zeros(5, dtype=torch.int32, device="cuda")
    pnp.scene_flow_device(d_xy.data_ptr(), d_next.data_ptr(), d_state.data_ptr(), d_n.data_ptr(), ch.d["z0"].data_ptr(), 640, ch.d["z1"].data_ptr(),
                          640, 640, 480, ch.cam, dr.FX, dr.FY, Rt.data_ptr(), pst.data_ptr())
    st.synchronize()
    pre, nxt, state = d_xy.cpu().numpy()[:n], d_next.cpu().numpy(), d_state.cpu().numpy()
    assert np.array_equal(state, fo.flow_check(ch.f0, ch.f1, pre, nxt, d_lk.cpu().numpy()))
    want = dr.tail(pre, nxt, state, n, F2.cpu().numpy(), fst.cpu().numpy(), Rt.cpu().numpy(), pst.cpu().numpy(), ch.z0, ch.z1, dr.CAM,
                   np.eye(3, 4, dtype=np.float32), dr.FX, dr.FY, np.eye(3, 4, dtype=np.float32))
    r, rm, kps, desc, labels, centers = res
    wrm, wave, wep, wst = dr.decide(want["match"], want["rpe"], want["tm"], labels, centers[:, 7], 15)
    orc = ob.Oracle()
    orc.detect(ch.f1)
    orc.gate(np.zeros((480, 640), np.uint8), labels, centers[:, 7].copy(), wrm)
    ko, do = orc.describe()
    for h in (det, lk, fmat, pnp):
        h.close()
    return n, want, (wrm, wave, wep, wst), (ko, do)


def test_whole_chain_removes_the_moving_block(gpu_lib, ob, synth):
    import torch
    s = torch.cuda.Stream()
    ch = _Chain(gpu_lib, synth, s.cuda_stream)
    ch.run()
    res = ch.outputs()
    n, want, (wrm, wave, wep, wst), (ko, do) = _chain_want(gpu_lib, ob, ch, res)
    r, rm, kps, desc, labels, centers = res
    want["epipolar"] = np.r_[want["epipolar"], r["epipolar"][n:]]  # the tail writes n entries; fetch read 1000
    _same(r, want, "chain tail")
    assert rm.tobytes() == wrm.tobytes() and r["ave_rpe"].tobytes() == wave.tobytes() and r["ep_num"].tobytes() == wep.tobytes()
    assert r["decide_status"] == wst
    assert kps.tobytes() == ko.tobytes() and desc.tobytes() == do.tobytes()
    assert want["status"] == 0 and want["counts"][4] > 0
    cid = centers[int(labels[232, 362]) - 1, 7]  # the block's centre in the current frame
    assert rm[cid] == 1, (cid, rm, wave, wep)


def test_whole_chain_replays_from_a_graph(gpu_lib, synth):
    import torch
    s = torch.cuda.Stream()
    ch = _Chain(gpu_lib, synth, s.cuda_stream)
    ch.run()
    eager = ch.outputs()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ch.run()
    for _ in range(2):
        ch.d["rm"].fill_(5)
        torch.cuda.synchronize()
        g.replay()
        got = ch.outputs()
        _same(got[0], eager[0], "graph tail")
        for a, b in zip(got[1:], eager[1:]):
            assert a.tobytes() == b.tobytes()
