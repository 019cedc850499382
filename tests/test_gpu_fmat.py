"""GPU: amos_fmat_* (cv::findFundamentalMat(FM_RANSAC) of Tracking::GetSceneFlowObj on the device) against the restatement in
tests/fmat_restatement.py: the 9 doubles of F, the inlier mask and the status {result, inliers, iterations, points} bit for bit."""
import os
import sys

import numpy as np
import pytest

import fmat_restatement as fr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
MAXP = 4096


@pytest.fixture(scope="module")
def fm(gpu_lib):
    h = gpu_lib.FundamentalRansac(max_points=MAXP, max_problems=64)
    yield h
    h.close()


def _run_batch(torch, fm, problems, select=None, max_iters=1000):
    """problems: list of (p1, p2); one launch; returns [(F, mask, status)] from the device."""
    counts = np.array([len(p) for p, _ in problems], np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    P1 = np.concatenate([p for p, _ in problems]).astype(np.float32).reshape(-1, 2)
    P2 = np.concatenate([q for _, q in problems]).astype(np.float32).reshape(-1, 2)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(p1=P1, p2=P2, off=offsets, cnt=counts).items()}
    d_sel = torch.from_numpy(select).cuda() if select is not None else None
    F = torch.full((len(problems), 9), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((len(problems), 4), -9, dtype=torch.int32, device="cuda")
    mask = torch.full((len(P1),), 7, dtype=torch.uint8, device="cuda")
    fm.ransac_device(len(problems), d["p1"].data_ptr(), d["p2"].data_ptr(), d["off"].data_ptr(), d["cnt"].data_ptr(),
                     d_sel.data_ptr() if d_sel is not None else None, F.data_ptr(), st.data_ptr(), mask.data_ptr(), max_iters=max_iters)
    torch.cuda.ExternalStream(fm.stream).synchronize()
    F, st, mask = F.cpu().numpy(), st.cpu().numpy(), mask.cpu().numpy()
    return [(F[i], mask[offsets[i]:offsets[i] + counts[i]], tuple(int(v) for v in st[i])) for i in range(len(problems))]


def _want(p1, p2, sel=None, max_iters=1000):
    s = np.ones(len(p1), bool) if sel is None else sel.astype(bool)
    F, m, st = fr.find_fundamental_ransac(p1[s], p2[s], max_iters=max_iters)
    mask = np.zeros(len(p1), np.uint8)
    mask[s] = m
    return F, mask, st


def _same(got, want, what):
    F, mask, st = got
    wF, wmask, wst = want
    assert st == tuple(wst), (what, st, wst)
    assert F.tobytes() == np.asarray(wF, np.float64).tobytes(), (what, F, wF)
    assert np.array_equal(mask, wmask), (what, int((mask != wmask).sum()))


CASES = [(15, 0.0, 0.0), (15, 0.3, 0.3), (16, 0.0, 0.3), (16, 0.3, 0.0), (100, 0.0, 0.0), (100, 0.3, 0.3), (100, 0.6, 0.0),
         (1000, 0.0, 0.3), (1000, 0.3, 0.0), (1000, 0.3, 0.3), (1000, 0.6, 0.3), (MAXP, 0.3, 0.3), (MAXP, 0.6, 0.0)]


@pytest.mark.parametrize("n,frac,noise", CASES)
def test_single_problem_equals_the_restatement(gpu_lib, fm, n, frac, noise):
    import torch
    p1, p2, _, _ = fr.two_view(np.random.default_rng(n * 7 + int(frac * 10) + int(noise * 10)), n, frac, noise)
    want = _want(p1, p2)
    _same(_run_batch(torch, fm, [(p1, p2)])[0], want, (n, frac, noise))
    assert want[2][0] == 1 and want[2][3] == n and want[2][1] >= 7


def test_special_inputs(gpu_lib, fm):
    import torch
    rng = np.random.default_rng(21)
    line = np.c_[rng.uniform(0, 640, 60), np.full(60, 240.0)].astype(np.float32)
    same = np.tile(np.float32([[100.5, 200.25]]), (40, 1))
    p10, q10, _, _ = fr.two_view(rng, 10)
    p3, q3, _, _ = fr.two_view(rng, 3)
    p, q, _, _ = fr.two_view(rng, 200, 0.6, 0.3)
    probs = [(line, line + np.float32(3)), (same, same), (p10, q10), (p3, q3)]
    got = _run_batch(torch, fm, probs)
    for g, (a, b), st in zip(got, probs, [(0, 0, 0, 60), (0, 0, 0, 40), (-1, 0, 0, 10), (0, 0, 0, 3)]):
        _same(g, _want(a, b), st)
        assert g[2] == st
    # max_iters = 5
    g = _run_batch(torch, fm, [(p, q)], max_iters=5)[0]
    _same(g, _want(p, q, max_iters=5), "max_iters")
    assert g[2][2] == 5
    # the synchronous host-pointer form gives the same
    F, mask, st = fm.ransac(p, q)
    _same((F.reshape(9), mask, tuple(int(v) for v in st)), _want(p, q), "sync")


def test_batch_equals_single_calls_and_is_reproducible(gpu_lib, fm):
    import torch
    rng = np.random.default_rng(22)
    probs, sels = [], []
    for i in range(24):
        n = int(rng.choice([5, 12, 15, 40, 300, 1000, 2000]))
        p, q, _, _ = fr.two_view(rng, n, float(rng.choice([0.0, 0.3, 0.5])), float(rng.choice([0.0, 0.3])))
        probs.append((p, q))
        sels.append((rng.random(n) < 0.9).astype(np.uint8))
    sel = np.concatenate(sels)
    batch = _run_batch(torch, fm, probs, select=sel)
    again = _run_batch(torch, fm, probs, select=sel)
    for i, ((p, q), s) in enumerate(zip(probs, sels)):
        one = _run_batch(torch, fm, [(p, q)], select=s)[0]
        for a, b in ((batch[i], one), (batch[i], again[i])):
            assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), i
        if i % 3 == 0:
            _same(batch[i], _want(p, q, s), ("batch", i))
        assert not batch[i][1][s == 0].any()


def _pair_want(pre, nxt, state):
    import flow_oracle as fo
    s = state != 0
    F1, _, st1 = fr.find_fundamental_ransac(pre[s], nxt[s])
    if st1[0] == 1:
        dd = fo.epipolar(F1, pre, nxt, state)
        keep = (s & (dd <= 0.5)).astype(np.uint8)
    else:
        keep = np.zeros(len(pre), np.uint8)
    F2, _, st2 = fr.find_fundamental_ransac(pre[keep != 0], nxt[keep != 0])
    return F1, F2, keep, np.array([st1, st2], np.int32)


def test_resident_scene_flow_chain(gpu_lib, ob, synth):
    """Tracking.cc:894-946 on the device: corners -> sub-pixel -> LK -> SAD / border check -> both findFundamentalMat calls with the
    epipolar filter between them; against the host chain of the oracles and the restatement."""
    import torch
    import flow_oracle as fo
    f0, f1 = synth.frame(9, 10), synth.frame(9, 11)
    want_xy = ob.corner_subpix(f0, ob.good_features_to_track(f0))
    want_next, want_st, _, _ = ob.lk_track(f0, f1, want_xy)
    want_state = fo.flow_check(f0, f1, want_xy, want_next, want_st)
    wF1, wF2, wkeep, wstatus = _pair_want(want_xy, want_next, want_state)
    det = gpu_lib.CornerDetector()
    lk = gpu_lib.LkTracker(640, 480, stream=det.stream)
    fm = gpu_lib.FundamentalRansac(max_points=1000, max_problems=1, stream=det.stream)
    st = torch.cuda.ExternalStream(det.stream)
    d0, d1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
    d_xy = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.good_features_device(d0.data_ptr(), 640, 640, 480, d_xy.data_ptr(), 1000, d_n.data_ptr())
    det.subpix_device(d0.data_ptr(), 640, 640, 480, d_xy.data_ptr(), count_ptr=d_n.data_ptr(), n=1000)
    st.synchronize()
    n = int(d_n.item())   # amos_lk_track_device takes a host count; the RANSACs read d_n
    assert n == len(want_xy)
    d_next = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    d_lk = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_state = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lk.track_device(d0.data_ptr(), 640, d1.data_ptr(), 640, d_xy.data_ptr(), n, d_next.data_ptr(), d_lk.data_ptr())
    gpu_lib.flow_check(det.stream, d0.data_ptr(), 640, d1.data_ptr(), 640, 640, 480, d_xy.data_ptr(), d_next.data_ptr(), d_lk.data_ptr(), n,
                       d_state.data_ptr())
    F1 = torch.zeros(9, dtype=torch.float64, device="cuda")
    F2 = torch.zeros(9, dtype=torch.float64, device="cuda")
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    status = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    fm.scene_flow_pair_device(d_xy.data_ptr(), d_next.data_ptr(), d_state.data_ptr(), d_n.data_ptr(), F1.data_ptr(), F2.data_ptr(), keep.data_ptr(),
                              status.data_ptr())
    st.synchronize()
    assert np.array_equal(d_state.cpu().numpy(), want_state)
    assert np.array_equal(status.cpu().numpy(), wstatus), (status.cpu().numpy(), wstatus)
    assert F1.cpu().numpy().tobytes() == wF1.tobytes() and F2.cpu().numpy().tobytes() == wF2.tobytes()
    assert np.array_equal(keep.cpu().numpy(), wkeep)
    assert wstatus[0, 0] == 1 and wstatus[1, 0] == 1 and wstatus[1, 3] == int(wkeep.sum()) > 0.5 * n
    fm.close()


def test_pair_call_replays_from_a_graph(gpu_lib):
    """The pair call captured once on one stream into a torch.cuda graph: replays equal the eager call, so nothing syncs with the host."""
    import torch
    rng = np.random.default_rng(23)
    pre, nxt, _, _ = fr.two_view(rng, 800, 0.3, 0.3)
    state = (rng.random(800) < 0.9).astype(np.uint8)
    s = torch.cuda.Stream()
    fm = gpu_lib.FundamentalRansac(max_points=1000, max_problems=1, stream=s.cuda_stream)
    d_pre, d_nxt, d_state = (torch.from_numpy(a).cuda() for a in (pre, nxt, state))
    d_n = torch.tensor([800], dtype=torch.int32, device="cuda")
    outs = [torch.zeros(9, dtype=torch.float64, device="cuda"), torch.zeros(9, dtype=torch.float64, device="cuda"),
            torch.zeros(800, dtype=torch.uint8, device="cuda"), torch.zeros((2, 4), dtype=torch.int32, device="cuda")]

    def call():
        fm.scene_flow_pair_device(d_pre.data_ptr(), d_nxt.data_ptr(), d_state.data_ptr(), d_n.data_ptr(), *(o.data_ptr() for o in outs))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()
    s.synchronize()
    eager = [o.cpu().clone() for o in outs]
    wF1, wF2, wkeep, wstatus = _pair_want(pre, nxt, state)
    assert eager[0].numpy().tobytes() == wF1.tobytes() and eager[1].numpy().tobytes() == wF2.tobytes()
    assert np.array_equal(eager[2].numpy(), wkeep) and np.array_equal(eager[3].numpy(), wstatus)
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
    fm.close()
