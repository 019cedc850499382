"""GPU: the scene-flow front (goodFeaturesToTrack -> cornerSubPix -> calcOpticalFlowPyrLK -> SAD / border check -> back-projection;
amos_corners.hip, amos_flow.hip) held to the CPU oracle AWAY from the one configuration the product calls: padded rows behind an
offset pointer, every window and level count, the iteration parameters, point counts that do not fill a work-group, dense and
chained corner selections, frames barely larger than the window, handles used twice.  Bit for bit like the other parity tests:
tobytes() equality for floats, array_equal for states and counts.

Every image goes to the device in a buffer whose rows are `width + 13` elements apart (odd, no multiple of 4), whose padding holds
a poison value that differs between the two images of a pair, and whose first pixel sits 3 elements behind the allocation start; the
oracle gets the contiguous array.  (For the uint8 frames 3 elements are 3 bytes; the float32 depth maps keep their 4-byte alignment.)

The shapes are the smallest at which the level / tile / tail logic still varies, so the whole module runs in seconds."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

f32 = np.float32
PAD, OFF = 13, 3
POISON_A, POISON_B = 0xA5, 0x5A


@pytest.fixture(scope="module")
def torch_gpu(gpu_lib):
    import torch
    return torch


class Strided:
    """A 2-D host array on the device with padded rows behind an offset pointer: .ptr, .stride (in elements)."""

    def __init__(self, torch, a, poison, pad=PAD):
        h, w = a.shape
        self.stride = w + pad
        host = np.full((h + 1) * self.stride, poison, a.dtype)  # one row extra: room for the offset
        host[OFF:OFF + h * self.stride].reshape(h, self.stride)[:, :w] = a
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + OFF * a.dtype.itemsize


# ------------------------------------------------------------------------------------------------------------------ LK

LK_FRAMES = [(97, 61), (47, 45), (23, 24)]   # (w, h)
LK_WINDOWS = [3, 5, 15, 21, 22]
LK_LEVELS = [0, 1, 5]
LK_STREAM = 33


def lk_points(w, h, n=203, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    pts = np.stack([rng.uniform(-5, w + 5, n), rng.uniform(-5, h + 5, n)], 1).astype(f32)
    k = min(50, n)
    pts[:k] = np.stack([rng.uniform(0, w, k), rng.uniform(0, h, k)], 1).round()  # integer positions: zero fractional weights
    return pts


def lk_pair(synth, w, h, stream=LK_STREAM):
    return synth.frame(stream, 4, h, w), synth.frame(stream, 5, h, w)


def lk_run(torch, lk, a, b, pts, pads=(PAD, PAD), **kw):
    """track on strided buffers; outputs carry three sentinel entries past the n points"""
    n = len(pts)
    A, B = Strided(torch, a, POISON_A, pads[0]), Strided(torch, b, POISON_B, pads[1])
    d_p = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    d_out = torch.full((n + 3, 2), -9.0, dtype=torch.float32, device="cuda")
    d_st = torch.full((n + 3,), 9, dtype=torch.uint8, device="cuda")
    d_err = torch.full((n + 3,), -9.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lk.track_device(A.ptr, A.stride, B.ptr, B.stride, d_p.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), d_err.data_ptr(), **kw)
    torch.cuda.ExternalStream(lk.stream).synchronize()
    return d_out.cpu().numpy(), d_st.cpu().numpy(), d_err.cpu().numpy()


def lk_assert_equal(got, want, what):
    (gout, gst, gerr), (wout, wst, werr) = got, want
    n = len(wst)
    assert np.array_equal(gst[:n], wst), what
    bad = np.nonzero((gout[:n] != wout).any(1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:3], gout[bad[:3]], wout[bad[:3]])
    assert gout[:n].tobytes() == wout.tobytes() and gerr[:n].tobytes() == werr.tobytes(), what
    assert (gout[n:] == -9).all() and (gst[n:] == 9).all() and (gerr[n:] == -9).all(), (what, "wrote past n")


def lk_case(torch, gpu_lib, ob, a, b, pts, win, max_level, pads=(PAD, PAD), **kw):
    """one handle, one call, against the oracle; returns the oracle's (top, tracked fraction)"""
    h, w = a.shape
    *want, top = ob.lk_track(a, b, pts, win=win, max_level=max_level, **kw)
    what = (w, h, win, max_level, kw)
    assert 0 < int(want[1].sum()) < len(pts), ("vacuous", what, int(want[1].sum()))  # the oracle alone tracks some and rejects some
    lk = gpu_lib.LkTracker(w, h, win_size=win, max_level=max_level)
    try:
        assert lk.levels == top, what
        lk_assert_equal(lk_run(torch, lk, a, b, pts, pads, **kw), want, what)
    finally:
        lk.close()
    return top, float(want[1].mean())


@pytest.mark.parametrize("win", LK_WINDOWS)
@pytest.mark.parametrize("w,h", LK_FRAMES)
def test_lk_window_level_grid(gpu_lib, ob, synth, torch_gpu, w, h, win):
    assert w > win and h > win  # (every frame of the grid is larger than every window)
    a, b = lk_pair(synth, w, h)
    pts = lk_points(w, h)
    tops = [lk_case(torch_gpu, gpu_lib, ob, a, b, pts, win, ml)[0] for ml in LK_LEVELS]
    assert tops[0] == 0 and tops[1] <= 1 and tops[1] <= tops[2] <= 4


def test_lk_top_level_7(gpu_lib, ob, synth, torch_gpu):
    """the last slot of the level table: 640 x 480, window 3, max_level 7 -> 5 x 4 pixels at the top"""
    a, b = lk_pair(synth, 640, 480)
    top, _ = lk_case(torch_gpu, gpu_lib, ob, a, b, lk_points(640, 480), 3, 7)
    assert top == 7


def test_lk_different_strides_in_a_pair(gpu_lib, ob, synth, torch_gpu):
    a, b = lk_pair(synth, 97, 61)
    lk_case(torch_gpu, gpu_lib, ob, a, b, lk_points(97, 61), 9, 3, pads=(PAD, 7))
    lk_case(torch_gpu, gpu_lib, ob, a, b, lk_points(97, 61), 22, 5, pads=(1, PAD))


LK_ITERATION = [(0, 0.01, 1e-4), (1, 0.0, 1e-4), (100, 0.0, 1e-4), (20, 0.3, 1e-4), (20, 0.01, 1e-2), (20, 0.01, 0.0)]


@pytest.mark.parametrize("max_count,epsilon,min_eig", LK_ITERATION)
def test_lk_iteration_parameters(gpu_lib, ob, synth, torch_gpu, max_count, epsilon, min_eig):
    a, b = lk_pair(synth, 97, 61)
    lk_case(torch_gpu, gpu_lib, ob, a, b, lk_points(97, 61), 9, 3, max_count=max_count, epsilon=epsilon, min_eig=min_eig)


def lk_tail_points(ob, a, b, win, max_level):
    """five points of the 203, ordered tracked, rejected, tracked, tracked, rejected: every prefix of 2 or more is non-vacuous"""
    h, w = a.shape
    pts = lk_points(w, h)
    st = ob.lk_track(a, b, pts, win=win, max_level=max_level)[1]
    good, bad = np.nonzero(st == 1)[0], np.nonzero(st == 0)[0]
    return pts[[good[0], bad[0], good[1], good[2], bad[1]]]


def test_lk_point_counts_below_a_work_group(gpu_lib, ob, synth, torch_gpu):
    """the work-group holds four waves, one point each: 1, 2, 3 points leave waves idle, 5 start a second group with one"""
    a, b = lk_pair(synth, 97, 61)
    five = lk_tail_points(ob, a, b, 9, 3)
    lk = gpu_lib.LkTracker(97, 61, win_size=9, max_level=3)
    for n in (1, 2, 3, 5):
        *want, _ = ob.lk_track(a, b, five[:n], win=9, max_level=3)
        assert want[1].tolist() == [1, 0, 1, 1, 0][:n]
        lk_assert_equal(lk_run(torch_gpu, lk, a, b, five[:n]), want, n)
    lk.close()


def test_lk_handle_reuse(gpu_lib, ob, synth, torch_gpu):
    """pair A, then pair B with other iteration parameters on the same handle: a stale pyramid or derivative border would show in B"""
    a0, a1 = lk_pair(synth, 97, 61)
    b0, b1 = lk_pair(synth, 97, 61, stream=34)
    pts = lk_points(97, 61)
    lk = gpu_lib.LkTracker(97, 61, win_size=9, max_level=3)
    *want_a, _ = ob.lk_track(a0, a1, pts, win=9, max_level=3)
    *want_b, _ = ob.lk_track(b0, b1, pts, win=9, max_level=3, max_count=7, epsilon=0.1, min_eig=1e-3)
    for want in (want_a, want_b):
        assert 0 < int(want[1].sum()) < len(pts)
    assert want_a[0].tobytes() != want_b[0].tobytes()
    lk_assert_equal(lk_run(torch_gpu, lk, a0, a1, pts), want_a, "A")
    lk_assert_equal(lk_run(torch_gpu, lk, b0, b1, pts, max_count=7, epsilon=0.1, min_eig=1e-3), want_b, "B after A")
    lk.close()


# ------------------------------------------------------------------------------------------------- goodFeaturesToTrack

GF_CAP = 2000
GF_NOISE = [(131, 97), (64, 48), (33, 9)]   # (w, h)
GF_DISTANCES = [1.0, 1.5, 2.5, 4.0, 8.0, 30.0]
GF_QUALITIES = [1e-6, 0.01, 0.3]
GF_MAX_CORNERS = [0, 25]


def noise_image(w, h, seed=0):
    return np.random.default_rng(100 * w + h + seed).integers(0, 256, (h, w), dtype=np.uint8)


def chain_image():
    """twenty 2 x 2 blobs of falling brightness on a 131 x 21 black image, 6 px apart: each blob's fate depends on the one before it"""
    img = np.zeros((21, 131), np.uint8)
    for i in range(20):
        img[10:12, 5 + 6 * i:7 + 6 * i] = 250 - 6 * i
    return img


def gf_case(torch, det, ob, img, what=None, **kw):
    """one good_features_device call on a strided buffer against the oracle: response plane, count, list; returns the oracle's list"""
    h, w = img.shape
    want_xy, want_R = ob.good_features_to_track(img, with_response=True, **kw)
    assert len(want_xy) <= GF_CAP
    S = Strided(torch, np.ascontiguousarray(img), POISON_A)
    d_xy = torch.full((GF_CAP + 1, 2), -1.0, dtype=torch.float32, device="cuda")
    d_n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d_R = torch.full((h * w + 1,), -3.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    det.good_features_device(S.ptr, S.stride, w, h, d_xy.data_ptr(), GF_CAP, d_n.data_ptr(), response_ptr=d_R.data_ptr(), **kw)
    torch.cuda.ExternalStream(det.stream).synchronize()
    what = (w, h, kw, what)
    R = d_R.cpu().numpy()
    assert R[:h * w].tobytes() == want_R.tobytes() and R[h * w] == -3.0, ("Harris response", what)
    n = int(d_n.item())
    xy = d_xy.cpu().numpy()
    assert n == len(want_xy), ("corner count", what, n, len(want_xy))
    assert xy[:n].tobytes() == want_xy.tobytes(), ("corner list", what)
    assert (xy[n:] == -1).all(), ("wrote past the count", what)
    assert det.candidate_count() >= n
    return want_xy


@pytest.mark.parametrize("w,h", GF_NOISE)
def test_corners_dense_noise(gpu_lib, ob, torch_gpu, w, h):
    img = noise_image(w, h)
    det = gpu_lib.CornerDetector(max_width=w, max_height=h)
    counts = {}
    for md in GF_DISTANCES:
        for q in GF_QUALITIES:
            for mc in GF_MAX_CORNERS:
                counts[md, q, mc] = len(gf_case(torch_gpu, det, ob, img, max_corners=mc, quality=q, min_distance=md))
    det.close()
    assert all(c >= 1 for c in counts.values())
    assert all(counts[md, q, 25] == min(25, counts[md, q, 0]) for md in GF_DISTANCES for q in GF_QUALITIES)
    if (w, h) != (33, 9):  # the selection really rejects, and lrint(2.5) = 2 cells are in use
        assert counts[2.5, 1e-6, 0] < counts[1.0, 1e-6, 0] and counts[8.0, 1e-6, 0] < counts[2.5, 1e-6, 0]
        assert counts[1.0, 1e-6, 0] > 100


@pytest.mark.parametrize("w,h", [(8, 8), (95, 8)])
def test_corners_smallest_frames(gpu_lib, ob, torch_gpu, w, h):
    img = noise_image(w, h)
    det = gpu_lib.CornerDetector(max_width=w, max_height=h)
    n = [len(gf_case(torch_gpu, det, ob, img, max_corners=0, quality=1e-6, min_distance=md)) for md in (1.0, 2.5)]
    det.close()
    assert n[0] >= 1


def test_corners_dependency_chain(gpu_lib, ob, torch_gpu):
    img = chain_image()
    det = gpu_lib.CornerDetector(max_width=131, max_height=21)
    dense = gf_case(torch_gpu, det, ob, img, max_corners=0, quality=1e-4, min_distance=1.0)
    chain = gf_case(torch_gpu, det, ob, img, max_corners=0, quality=1e-4, min_distance=7.0)
    det.close()
    assert len(dense) == 80
    # every second blob survives: blob 2k is kept because blob 2k - 1 was dropped because blob 2k - 2 was kept ...: twenty dependent rounds
    assert len(chain) == 10 and chain[:, 0].tolist() == [6.0 + 12 * i for i in range(10)]


def test_corners_none_to_find(gpu_lib, ob, torch_gpu):
    step = np.zeros((48, 64), np.uint8)
    step[:, 32:] = 200
    assert ob.corner_harris(step).max() == 0 and ob.corner_harris(step).min() < 0  # no response above zero, some below
    det = gpu_lib.CornerDetector(max_width=64, max_height=48)
    for img in (step, np.full((48, 64), 77, np.uint8)):
        for md in (1.0, 8.0):
            assert len(gf_case(torch_gpu, det, ob, img, max_corners=0, quality=0.01, min_distance=md)) == 0
    det.close()


def test_corners_handle_reuse_smaller_after_larger(gpu_lib, ob, torch_gpu):
    """stale cell lists, candidate counts or response rows of the larger frame would show in the smaller one"""
    det = gpu_lib.CornerDetector(max_width=131, max_height=97)
    for w, h in ((131, 97), (33, 9), (64, 48)):
        for md in (1.0, 4.0):
            assert len(gf_case(torch_gpu, det, ob, noise_image(w, h), max_corners=0, quality=1e-6, min_distance=md)) >= 1
    det.close()


# -------------------------------------------------------------------------------------------------------- cornerSubPix

def subpix_points(w, h, n=100, seed=0):
    """the corner and edge points of the 140 x 100 border test scaled to the frame, then n random ones"""
    rng = np.random.default_rng(10 * w + h + seed)
    border = np.array([[1, 1], [138, 1], [1, 98], [138, 98], [70, 1], [1, 50], [138.5, 50.25], [69.5, 98.75], [0.25, 0.25]], f32)
    border = (border * [(w - 1) / 139.0, (h - 1) / 99.0]).astype(f32)
    return np.concatenate([border, (rng.random((n, 2)) * [w - 1, h - 1]).astype(f32)])


def subpix_case(torch, det, ob, img, pts, win, max_count=20, epsilon=0.03):
    h, w = img.shape
    n = len(pts)
    want = ob.corner_subpix(img, pts, win, max_count, epsilon)
    S = Strided(torch, np.ascontiguousarray(img), POISON_A)
    d_xy = torch.full((n + 2, 2), -5.0, dtype=torch.float32, device="cuda")
    d_xy[:n] = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    torch.cuda.synchronize()
    det.subpix_device(S.ptr, S.stride, w, h, d_xy.data_ptr(), n=n, win=win, max_count=max_count, epsilon=epsilon)
    torch.cuda.ExternalStream(det.stream).synchronize()
    got = d_xy.cpu().numpy()
    what = (w, h, win, n, max_count, epsilon)
    bad = np.nonzero((got[:n] != want).any(1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:3], got[bad[:3]], want[bad[:3]])
    assert got[:n].tobytes() == want.tobytes(), what
    assert (got[n:] == -5).all(), ("wrote past n", what)
    return want


@pytest.fixture(scope="module")
def subpix_det(gpu_lib):
    det = gpu_lib.CornerDetector(max_width=140, max_height=100)
    yield det
    det.close()


@pytest.mark.parametrize("win", [1, 2, 14, 15])
def test_subpix_windows(subpix_det, ob, synth, torch_gpu, win):
    """the extreme windows, 15 being the largest the header admits (three corners per work-group: four do not fit the LDS), on a
    140 x 100 frame and on the smallest legal one"""
    img = synth.frame(7, 3, 100, 140)
    pts = subpix_points(140, 100)
    want = subpix_case(torch_gpu, subpix_det, ob, img, pts, win)
    assert (want != pts).any(1).sum() > len(pts) // 10  # the refinement moves points (the others left their window and were put back)
    s = 2 * win + 5
    subpix_case(torch_gpu, subpix_det, ob, synth.frame(7, 3, s, s), subpix_points(s, s), win)


@pytest.mark.parametrize("win", [2, 10, 15])
def test_subpix_tails(subpix_det, ob, synth, torch_gpu, win):
    img = synth.frame(7, 3, 100, 140)
    pts = subpix_points(140, 100, 5, seed=1)[9:]
    for n in (1, 2, 3, 5):
        subpix_case(torch_gpu, subpix_det, ob, img, pts[:n], win)


def test_subpix_termination(subpix_det, ob, synth, torch_gpu):
    img = synth.frame(7, 3, 100, 140)
    pts = subpix_points(140, 100)
    one = subpix_case(torch_gpu, subpix_det, ob, img, pts, 14, 1, 0.0)
    many = subpix_case(torch_gpu, subpix_det, ob, img, pts, 14, 100, 1e-4)
    assert one.tobytes() != many.tobytes()


# ----------------------------------------------------------------------------------------- the point kernels of amos_flow.hip

FLOW_W, FLOW_H = 67, 43
FLOW_COUNTS = [1, 255, 256, 257]
SAD_MAX = 9 * 255


def flow_scene(synth):
    """257 point pairs on a 67 x 43 frame pair.  The first 17: one pair inside (kept, so that n = 1 keeps), then pre and next on both sides
    of each of the four 5-px limits (int() truncates: 4.99 is out, 5.0 in, 61.99 in, 62.0 out; 37.99 in, 38.0 out).  Then a black patch
    against a white one: the largest sum of absolute differences nine 8-bit pixels can have, 2295.  THE REFERENCE'S LIMIT OF 2520 LIES
    ABOVE IT (Tracking.cc:917), so no pair is ever rejected by it; the kernel and the oracle restate that faithfully and this pair pins
    the comparison from below (a limit anywhere under 2295 rejects it).  It follows that no pixel can change a state: what the strided
    frames hold flow_check to is the limit and reads that stay inside the buffers, not the row pitch (a kernel built with the width for
    the pitch passed this test; the same change fails every corner, sub-pixel, LK and scene-flow test of this module)."""
    rng = np.random.default_rng(5)
    last, cur = synth.frame(31, 4, FLOW_H, FLOW_W).copy(), synth.frame(31, 5, FLOW_H, FLOW_W).copy()
    last[19:24, 29:34], cur[19:24, 29:34] = 0, 255
    n = 257
    pre = np.stack([rng.uniform(-3, FLOW_W + 3, n), rng.uniform(-3, FLOW_H + 3, n)], 1).astype(f32)
    nxt = (pre + np.array([2.0, 1.0], f32) + rng.normal(0, 0.7, (n, 2))).astype(f32)
    mid = [30.5, 20.5]
    edge = [[4.99, 20], [5.0, 20], [61.99, 20], [62.0, 20], [30, 4.99], [30, 5.0], [30, 37.99], [30, 38.0]]
    pre[0], nxt[0] = [12.25, 30.5], [13.5, 31.0]
    pre[1:9], nxt[1:9] = edge, mid
    pre[9:17], nxt[9:17] = mid, edge
    pre[17], nxt[17] = [31.0, 21.0], [31.9, 21.2]
    state = (rng.random(n) < 0.9).astype(np.uint8)
    state[:18] = 1
    return last, cur, pre, nxt, state


@pytest.mark.parametrize("n", FLOW_COUNTS)
def test_flow_check_tails_strided(gpu_lib, synth, torch_gpu, n):
    import flow_oracle as fo
    torch = torch_gpu
    last, cur, pre, nxt, state = flow_scene(synth)
    want = fo.flow_check(last, cur, pre[:n], nxt[:n], state[:n])
    assert want[0] == 1 and (n == 1 or 0 < want.sum() < n)
    d_pre, d_nxt, d_state = (torch.from_numpy(np.ascontiguousarray(a[:n])).cuda() for a in (pre, nxt, state))
    for pads in ((PAD, PAD), (PAD, 7)):  # the second: the two frames of the pair have different strides
        A, B = Strided(torch, last, POISON_A, pads[0]), Strided(torch, cur, POISON_B, pads[1])
        out = torch.full((n + 3,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu_lib.flow_check(torch.cuda.current_stream().cuda_stream, A.ptr, A.stride, B.ptr, B.stride, FLOW_W, FLOW_H, d_pre.data_ptr(), d_nxt.data_ptr(),
                           d_state.data_ptr(), n, out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], want) and (got[n:] == 7).all(), pads


@pytest.mark.parametrize("with_state", [True, False])
@pytest.mark.parametrize("n", FLOW_COUNTS)
def test_flow_epipolar_tails(gpu_lib, synth, torch_gpu, n, with_state):
    import flow_oracle as fo
    torch = torch_gpu
    _, _, pre, nxt, state = flow_scene(synth)
    state = state.copy()
    state[0] = 1
    state[3::5] = 0
    F = np.array([[1e-9, 2e-9, 1.0], [-3e-9, 1e-9, -2.0], [-1.0, 2.0, 1e-4]], np.float64)
    want = fo.epipolar(F, pre[:n], nxt[:n], state[:n] if with_state else None)
    assert (want >= 0).any() and (not with_state or n == 1 or (want == -1).any())
    d_F, d_pre, d_nxt, d_state = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (F, pre[:n], nxt[:n], state[:n]))
    dd = torch.full((n + 3,), -77.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu_lib.flow_epipolar(torch.cuda.current_stream().cuda_stream, d_F.data_ptr(), d_pre.data_ptr(), d_nxt.data_ptr(), d_state.data_ptr() if with_state else None,
                          n, dd.data_ptr())
    torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert got[:n].tobytes() == want.tobytes() and (got[n:] == -77.0).all()


def scene_flow_inputs(gpu_lib):
    """depth maps of 67 x 43 with about a tenth of the depths invalid; every match position INSIDE the maps (the entry point's contract)"""
    rng = np.random.default_rng(3)
    n = 257
    pre = np.stack([rng.uniform(0, FLOW_W - 0.1, n), rng.uniform(0, FLOW_H - 0.1, n)], 1).astype(f32)
    cur = np.clip(pre + rng.normal(0, 2, (n, 2)), 0, [FLOW_W - 0.1, FLOW_H - 0.1]).astype(f32)
    pre[0], cur[0] = [33.3, 21.7], [35.1, 22.2]
    pre[1], cur[1] = [0.0, 0.0], [FLOW_W - 0.1, FLOW_H - 0.1]   # the map's corners
    assert (pre >= 0).all() and (cur >= 0).all() and (pre.astype(int) < [FLOW_W, FLOW_H]).all() and (cur.astype(int) < [FLOW_W, FLOW_H]).all()
    yy, xx = np.mgrid[0:FLOW_H, 0:FLOW_W]
    d_last = (1.5 + 0.5 * np.sin(xx / 9.0) + 0.3 * np.cos(yy / 6.0)).astype(f32)
    d_cur = (d_last + 0.02).astype(f32)
    d_last[rng.random(d_last.shape) < 0.05] = 0
    d_cur[rng.random(d_cur.shape) < 0.05] = -1.0
    d_last[21, 33] = 1.75  # pair 0 is valid, so that n = 1 computes
    d_cur[22, 35] = 1.5
    th = 0.03
    Rlw = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], f32)
    Tlw = np.concatenate([Rlw, np.array([[0.1], [-0.05], [0.2]], f32)], 1)
    Rwc = Rlw.T.copy()
    Ow = np.array([-0.08, 0.04, -0.25], f32)
    cam = gpu_lib.SceneFlowCamera(33.1, 20.6, 1 / 53.4, 1 / 53.9)
    for i, v in enumerate(Tlw.reshape(-1)):
        cam.Tlw[i] = float(v)
    for i, v in enumerate(Rwc.reshape(-1)):
        cam.Rwc[i] = float(v)
    for i, v in enumerate(Ow):
        cam.Ow[i] = float(v)
    return d_last, d_cur, pre, cur, cam, Tlw, Rwc, Ow


@pytest.mark.parametrize("n", FLOW_COUNTS)
def test_scene_flow_tails_strided(gpu_lib, torch_gpu, n):
    import flow_oracle as fo
    torch = torch_gpu
    d_last, d_cur, pre, cur, cam, Tlw, Rwc, Ow = scene_flow_inputs(gpu_lib)
    want = fo.scene_flow(d_last, d_cur, pre[:n], cur[:n], f32(cam.cx), f32(cam.cy), f32(cam.invfx), f32(cam.invfy), Tlw, Rwc, Ow)
    assert want[0, 7] == 1 and (n == 1 or 0.7 < want[:, 7].mean() < 0.97) and want[want[:, 7] > 0, 6].max() > 0.01
    d_pre, d_cur_xy = (torch.from_numpy(np.ascontiguousarray(a[:n])).cuda() for a in (pre, cur))
    for pads in ((PAD, PAD), (PAD, 7)):  # strides in floats, as include/amos_frontend.h states; poisons are plausible depths
        A, B = Strided(torch, d_last, f32(7.5), pads[0]), Strided(torch, d_cur, f32(5.5), pads[1])
        out = torch.full((n + 1, 8), -4.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gpu_lib.flow_scene_flow(torch.cuda.current_stream().cuda_stream, A.ptr, A.stride, B.ptr, B.stride, d_pre.data_ptr(), d_cur_xy.data_ptr(), n, cam,
                                out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bad = np.nonzero((got[:n] != want).any(1))[0]
        assert len(bad) == 0, (pads, len(bad), got[bad[:2]].tolist(), want[bad[:2]].tolist())
        assert got[:n].tobytes() == want.tobytes() and (got[n:] == -4.0).all(), pads


# ------------------------------------------------------------------------------------------------------- refused calls

def test_refused_calls(gpu_lib, torch_gpu):
    """Strides below the width, min_distance / quality / sub-pixel windows outside the documented ranges, frames too small for the window:
    AMOS_ERR_INVALID before anything is launched (the buffers are real and large enough all the same).  What needs no handle is in
    tests/test_scene_flow_sweep_cpu.py."""
    torch = torch_gpu
    img = torch.zeros((100, 140), dtype=torch.uint8, device="cuda")
    xy = torch.zeros((64, 2), dtype=torch.float32, device="cuda")
    out = torch.zeros((64, 2), dtype=torch.float32, device="cuda")
    st = torch.zeros(64, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    invalid = dict(match=r"rc=-1")
    lk = gpu_lib.LkTracker(140, 100, win_size=9, max_level=3)
    for s0, s1 in ((139, 140), (140, 139), (0, 140)):
        with pytest.raises(gpu_lib.AmosError, **invalid):
            lk.track_device(img.data_ptr(), s0, img.data_ptr(), s1, xy.data_ptr(), 64, out.data_ptr(), st.data_ptr())
    with pytest.raises(gpu_lib.AmosError, **invalid):
        lk.track_device(img.data_ptr(), 140, img.data_ptr(), 140, xy.data_ptr(), -1, out.data_ptr(), st.data_ptr())
    lk.close()
    det = gpu_lib.CornerDetector(max_width=140, max_height=100)
    frame = dict(stride=140, width=140, height=100)
    for bad in (dict(stride=139), dict(width=141), dict(height=101), dict(min_distance=0.5), dict(min_distance=2000.0), dict(quality=0.0), dict(quality=-1.0)):
        a = {**frame, **{k: v for k, v in bad.items() if k in frame}}
        kw = {k: v for k, v in bad.items() if k not in frame}
        with pytest.raises(gpu_lib.AmosError, **invalid):
            det.good_features_device(img.data_ptr(), a["stride"], a["width"], a["height"], xy.data_ptr(), 64, n.data_ptr(), **kw)
    for win in (0, 16, -1):
        with pytest.raises(gpu_lib.AmosError, **invalid):
            det.subpix_device(img.data_ptr(), 140, 140, 100, xy.data_ptr(), n=64, win=win)
    for win in (1, 10, 15):  # a frame of 2 win + 4 is one pixel too small, in either direction
        for w, h in ((2 * win + 4, 100), (140, 2 * win + 4)):
            with pytest.raises(gpu_lib.AmosError, **invalid):
                det.subpix_device(img.data_ptr(), 140, w, h, xy.data_ptr(), n=64, win=win)
    with pytest.raises(gpu_lib.AmosError, **invalid):
        det.subpix_device(img.data_ptr(), 139, 140, 100, xy.data_ptr(), n=64)
    det.close()
