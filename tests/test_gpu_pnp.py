"""GPU: amos_pnp_* (cv::solvePnPRansac(SOLVEPNP_P3P) + EPnP refit of Tracking::GetSceneFlowObj on the device) against the restatement in
tests/pnp_restatement.py: the 12 doubles of R | t, the inlier mask and the status {result, inliers, iterations, points, refit} bit for bit."""
import os
import sys

import numpy as np
import pytest

import pnp_restatement as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
MAXP = 4096
K = pr.K_TUM


@pytest.fixture(scope="module")
def pnp(gpu_lib):
    h = gpu_lib.PnpRansac(max_points=MAXP, max_problems=64)
    yield h
    h.close()


def _run_batch(torch, pnp, problems, select=None, max_iters=500):
    """problems: list of (obj, img); one launch; returns [(Rt, mask, status)] from the device."""
    counts = np.array([len(o) for o, _ in problems], np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    O = np.concatenate([o for o, _ in problems]).astype(np.float32).reshape(-1, 3)
    I = np.concatenate([i for _, i in problems]).astype(np.float32).reshape(-1, 2)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(o=O, i=I, off=offsets, cnt=counts).items()}
    d_sel = torch.from_numpy(select).cuda() if select is not None else None
    Rt = torch.full((len(problems), 12), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((len(problems), 5), -9, dtype=torch.int32, device="cuda")
    mask = torch.full((len(O),), 7, dtype=torch.uint8, device="cuda")
    pnp.ransac_device(len(problems), d["o"].data_ptr(), d["i"].data_ptr(), d["off"].data_ptr(), d["cnt"].data_ptr(),
                      d_sel.data_ptr() if d_sel is not None else None, *K, Rt.data_ptr(), st.data_ptr(), mask.data_ptr(), max_iters=max_iters)
    torch.cuda.ExternalStream(pnp.stream).synchronize()
    Rt, st, mask = Rt.cpu().numpy(), st.cpu().numpy(), mask.cpu().numpy()
    return [(Rt[i], mask[offsets[i]:offsets[i] + counts[i]], tuple(int(v) for v in st[i])) for i in range(len(problems))]


def _want(obj, img, sel=None, max_iters=500):
    s = np.ones(len(obj), bool) if sel is None else sel.astype(bool)
    Rt, m, st = pr.solve_pnp_ransac(obj[s], img[s], *K, max_iters=max_iters)
    mask = np.zeros(len(obj), np.uint8)
    mask[s] = m
    return Rt, mask, st


def _same(got, want, what):
    Rt, mask, st = got
    wRt, wmask, wst = want
    assert st == tuple(wst), (what, st, wst)
    assert Rt.tobytes() == np.asarray(wRt, np.float64).tobytes(), (what, Rt, wRt)
    assert np.array_equal(mask, wmask), (what, int((mask != wmask).sum()))


CASES = [(4, 0.0, 0.0), (5, 0.0, 0.0), (5, 0.0, 0.05), (15, 0.0, 0.05), (15, 0.3, 0.05), (100, 0.0, 0.0), (100, 0.3, 0.05), (100, 0.5, 0.2),
         (1000, 0.0, 0.05), (1000, 0.3, 0.05), (1000, 0.5, 0.05), (1000, 0.6, 0.1), (MAXP, 0.3, 0.05), (MAXP, 0.5, 0.0)]


@pytest.mark.parametrize("n,frac,noise", CASES)
def test_single_problem_equals_the_restatement(gpu_lib, pnp, n, frac, noise):
    import torch
    obj, img, _, _ = pr.scene(np.random.default_rng(n * 7 + int(frac * 10) + int(noise * 100)), n, frac, noise)
    want = _want(obj, img)
    _same(_run_batch(torch, pnp, [(obj, img)])[0], want, (n, frac, noise))
    assert want[2][0] == 1 and want[2][3] == n


def test_special_inputs(gpu_lib, pnp):
    import torch
    rng = np.random.default_rng(41)
    o3, i3, _, _ = pr.scene(rng, 3)
    o4, i4, _, _ = pr.scene(rng, 4)
    o4[1] = o4[0]                                # 4 points, two identical: the direct P3P call has no model
    same_o = np.tile(np.float32([[0.5, 0.2, 3.0]]), (30, 1))
    same_i = np.tile(np.float32([[300.5, 200.25]]), (30, 1))
    op, ip, _, _ = pr.scene(rng, 300, planar=True)   # a wall
    probs = [(o3, i3), (o4, i4), (same_o, same_i), (op, ip)]
    got = _run_batch(torch, pnp, probs)
    for g, (a, b) in zip(got, probs):
        _same(g, _want(a, b), g[2])
    assert got[0][2] == (-1, 0, 0, 3, 0) and got[1][2][0] == 0 and got[2][2][0] == 0 and got[3][2][0] == 1
    # max_iters = 5 and the synchronous host-pointer form
    o, i, _, _ = pr.scene(rng, 200, 0.6, 0.05)
    g = _run_batch(torch, pnp, [(o, i)], max_iters=5)[0]
    _same(g, _want(o, i, max_iters=5), "max_iters")
    assert g[2][2] == 5
    Rt, mask, st = pnp.ransac(o, i, *K)
    _same((Rt, mask, tuple(int(v) for v in st)), _want(o, i), "sync")


def test_batch_equals_single_calls_and_is_reproducible(gpu_lib, pnp):
    import torch
    rng = np.random.default_rng(42)
    probs, sels = [], []
    for i in range(64):
        n = int(rng.choice([3, 4, 6, 15, 40, 300, 1000, 2000]))
        o, im, _, _ = pr.scene(rng, n, float(rng.choice([0.0, 0.3, 0.5])), float(rng.choice([0.0, 0.05])))
        probs.append((o, im))
        sels.append((rng.random(n) < 0.9).astype(np.uint8))
    sel = np.concatenate(sels)
    batch = _run_batch(torch, pnp, probs, select=sel)
    again = _run_batch(torch, pnp, probs, select=sel)
    for i, ((o, im), s) in enumerate(zip(probs, sels)):
        for a, b in ((batch[i], again[i]),):
            assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), i
        if i % 4 == 0:
            one = _run_batch(torch, pnp, [(o, im)], select=s)[0]
            assert one[2] == batch[i][2] and one[0].tobytes() == batch[i][0].tobytes() and np.array_equal(one[1], batch[i][1]), i
        if i % 8 == 0:
            _same(batch[i], _want(o, im, s), ("batch", i))
        assert not batch[i][1][s == 0].any()


def test_scorer_reproduces_the_mask(gpu_lib, pnp):
    """amos_flow_pnp_score_device on the returned R | t: its inlier mask is the returned mask when the RANSAC model is returned (the
    n == 4 direct call or a non-finite refit); with the EPnP refit it is the refit's own inlier set, which holds every RANSAC inlier here."""
    import torch
    obj, img, _, _ = pr.scene(np.random.default_rng(43), 1000, 0.3, 0.05)
    Rt, mask, st = _run_batch(torch, pnp, [(obj, img)])[0]
    assert st[0] == 1 and st[4] == 1
    d_Rt, d_o, d_i = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (Rt, obj, img))
    inl = torch.zeros(1, dtype=torch.int32, device="cuda")
    m = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    gpu_lib.flow_pnp_score(torch.cuda.current_stream().cuda_stream, d_Rt.data_ptr(), 1, d_o.data_ptr(), d_i.data_ptr(), 1000, *K, 0.4, None,
                           inl.data_ptr(), m.data_ptr())
    torch.cuda.synchronize()
    m = m.cpu().numpy()
    assert np.array_equal(m, (pr.errors(Rt, obj, img, *K) <= np.float32(0.16)).astype(np.uint8))
    assert (m[mask != 0] == 1).all()
    # the 4-point call returns the P3P model itself: the scorer gives back its mask exactly
    o4, i4, _, _ = pr.scene(np.random.default_rng(44), 4)
    Rt4, mask4, st4 = _run_batch(torch, pnp, [(o4, i4)])[0]
    d_Rt, d_o, d_i = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (Rt4, o4, i4))
    m = torch.zeros(4, dtype=torch.uint8, device="cuda")
    gpu_lib.flow_pnp_score(torch.cuda.current_stream().cuda_stream, d_Rt.data_ptr(), 1, d_o.data_ptr(), d_i.data_ptr(), 4, *K, 0.4, None,
                           inl.data_ptr(), m.data_ptr())
    torch.cuda.synchronize()
    assert st4[0] == 1 and np.array_equal(m.cpu().numpy(), mask4)


def _camera(gpu_lib):
    cam = gpu_lib.SceneFlowCamera(320.1, 247.6, 1 / 535.4, 1 / 539.2)
    for i, v in enumerate(np.eye(3, 4, dtype=np.float32).reshape(-1)):
        cam.Tlw[i] = float(v)
    for i, v in enumerate(np.eye(3, dtype=np.float32).reshape(-1)):
        cam.Rwc[i] = float(v)
    return cam


FX, FY = float(np.float32(535.4)), float(np.float32(539.2))


def _chain_want(cam, d_last, d_cur, pre, nxt, state):
    """Tracking.cc:955-1007 on the host: the oracle's back-projection for the lists, then the restatement."""
    import flow_oracle as fo
    s = state != 0
    mp, mc = pre[s], nxt[s]
    sf = fo.scene_flow(d_last, d_cur, mp, mc, np.float32(cam.cx), np.float32(cam.cy), np.float32(cam.invfx), np.float32(cam.invfy),
                       np.array(cam.Tlw, np.float32), np.array(cam.Rwc, np.float32), np.array(cam.Ow, np.float32))
    valid = sf[:, 7] > 0
    obj = np.where(valid[:, None], sf[:, :3], 0).astype(np.float32)
    img = np.where(valid[:, None], mc, 0).astype(np.float32)
    Rt, m, st = pr.solve_pnp_ransac(obj, img, FX, FY, float(np.float32(cam.cx)), float(np.float32(cam.cy)))
    mask = np.zeros(len(pre), np.uint8)
    mask[s] = m
    return Rt, mask, np.array(st, np.int32)


def test_resident_scene_flow_chain(gpu_lib, ob, synth):
    """Tracking.cc:894-1007 on the device: corners -> sub-pixel -> LK -> SAD / border check -> solvePnPRansac on the lists built from the
    depth maps (a wall at constant depth, last pose I | 0; frame k + 1 is frame k shifted by (2, 1) px: a pure translation)."""
    import torch
    import flow_oracle as fo
    f0, f1 = synth.frame(9, 10), synth.frame(9, 11)
    want_xy = ob.corner_subpix(f0, ob.good_features_to_track(f0))
    want_next, want_st, _, _ = ob.lk_track(f0, f1, want_xy)
    want_state = fo.flow_check(f0, f1, want_xy, want_next, want_st)
    depth = np.full((480, 640), 2.0, np.float32)
    depth[:40, :] = 0   # a band without depth: (0,0,0) -> (0,0) entries stay in the list
    cam = _camera(gpu_lib)
    wRt, wmask, wst = _chain_want(cam, depth, depth, want_xy, want_next, want_state)
    det = gpu_lib.CornerDetector()
    lk = gpu_lib.LkTracker(640, 480, stream=det.stream)
    pnp = gpu_lib.PnpRansac(max_points=1000, max_problems=1, stream=det.stream)
    st = torch.cuda.ExternalStream(det.stream)
    d0, d1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
    d_depth = torch.from_numpy(depth).cuda()
    d_xy = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.good_features_device(d0.data_ptr(), 640, 640, 480, d_xy.data_ptr(), 1000, d_n.data_ptr())
    det.subpix_device(d0.data_ptr(), 640, 640, 480, d_xy.data_ptr(), count_ptr=d_n.data_ptr(), n=1000)
    st.synchronize()
    n = int(d_n.item())
    assert n == len(want_xy)
    d_next = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    d_lk = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_state = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lk.track_device(d0.data_ptr(), 640, d1.data_ptr(), 640, d_xy.data_ptr(), n, d_next.data_ptr(), d_lk.data_ptr())
    gpu_lib.flow_check(det.stream, d0.data_ptr(), 640, d1.data_ptr(), 640, 640, 480, d_xy.data_ptr(), d_next.data_ptr(), d_lk.data_ptr(), n,
                       d_state.data_ptr())
    Rt = torch.full((12,), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.zeros(5, dtype=torch.int32, device="cuda")
    mask = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    pnp.scene_flow_device(d_xy.data_ptr(), d_next.data_ptr(), d_state.data_ptr(), d_n.data_ptr(), d_depth.data_ptr(), 640, d_depth.data_ptr(), 640,
                          640, 480, cam, FX, FY, Rt.data_ptr(), status.data_ptr(), mask.data_ptr())
    st.synchronize()
    assert np.array_equal(d_state.cpu().numpy(), want_state)
    assert np.array_equal(status.cpu().numpy(), wst), (status.cpu().numpy(), wst)
    assert Rt.cpu().numpy().tobytes() == np.asarray(wRt, np.float64).tobytes()
    assert np.array_equal(mask.cpu().numpy(), wmask)
    assert wst[0] == 1 and wst[1] > 0.5 * int((want_state != 0).sum())
    pnp.close()


def test_scene_flow_call_replays_from_a_graph(gpu_lib):
    """amos_pnp_scene_flow_device captured once into a torch.cuda graph: replays equal the eager call and the host chain."""
    import torch
    rng = np.random.default_rng(45)
    n = 800
    pre = np.c_[rng.uniform(10, 630, n), rng.uniform(10, 470, n)].astype(np.float32)
    nxt = (pre + np.float32([2.0, 1.0]) + rng.normal(0, 0.05, (n, 2))).astype(np.float32)
    nxt[rng.random(n) < 0.3] += np.float32(25.0)
    nxt = np.clip(nxt, 0, [639.9, 479.9]).astype(np.float32)
    state = (rng.random(n) < 0.9).astype(np.uint8)
    yy, xx = np.mgrid[0:480, 0:640]
    depth = (2.0 + 0.3 * np.sin(xx / 80.0)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.05] = 0
    cam = _camera(gpu_lib)
    s = torch.cuda.Stream()
    pnp = gpu_lib.PnpRansac(max_points=1000, max_problems=1, stream=s.cuda_stream)
    d_pre, d_nxt, d_state, d_depth = (torch.from_numpy(a).cuda() for a in (pre, nxt, state, depth))
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    outs = [torch.zeros(12, dtype=torch.float64, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda"),
            torch.zeros(n, dtype=torch.uint8, device="cuda")]

    def call():
        pnp.scene_flow_device(d_pre.data_ptr(), d_nxt.data_ptr(), d_state.data_ptr(), d_n.data_ptr(), d_depth.data_ptr(), 640, d_depth.data_ptr(),
                              640, 640, 480, cam, FX, FY, *(o.data_ptr() for o in outs))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()
    s.synchronize()
    eager = [o.cpu().clone() for o in outs]
    wRt, wmask, wst = _chain_want(cam, depth, depth, pre, nxt, state)
    assert eager[0].numpy().tobytes() == np.asarray(wRt, np.float64).tobytes()
    assert np.array_equal(eager[1].numpy(), wst) and np.array_equal(eager[2].numpy(), wmask)
    assert wst[0] == 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a.cpu(), b)
    pnp.close()
