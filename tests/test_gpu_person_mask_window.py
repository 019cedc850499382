"""k_person_mask with its staging rows derived from the scale and the detections culled by their crop rectangles
(amos_mask_person_window_mode 1, amos_mask_person_mask_rects_device) against the earlier form (mode 0: six staging rows, every flagged
detection everywhere), byte for byte, and once against a numpy restatement.  138 x 138 -> 640 x 480 is the network's case (a third of its
16-row tiles touch seven source rows); 10 x 10 -> 37 x 53 and n = 17 take the per-thread gathers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rects(n, ph, pw):
    """(x0, x1, y0, y1) per detection, mask pixels: empty, one pixel, the whole image, one touching each border, fractional ones inside"""
    kinds = [(4.0, 4.0, 2.0, 7.0),                                   # empty along x
             (5.0, 6.0, 7.0, 8.0),                                   # one pixel
             (0.0, float(pw), 0.0, float(ph)),                       # everything
             (0.0, 3.0, 1.0, ph - 1.0),                              # left border
             (pw - 3.0, float(pw), 1.0, ph - 1.0),                   # right border
             (1.0, pw - 1.0, 0.0, 2.0),                              # top border
             (1.0, pw - 1.0, ph - 2.0, float(ph)),                   # bottom border
             (0.3 * pw + 0.4, 0.7 * pw + 0.7, 0.2 * ph + 0.1, 0.6 * ph + 0.5),
             (0.5 * pw, 0.5 * pw + 1.5, 0.0, float(ph)),             # a thin column
             (0.0, float(pw), 0.45 * ph, 0.45 * ph + 1.2),           # a thin row
             (3.0, 2.0, 5.0, 1.0)]                                   # inverted: empty
    return np.array([kinds[i % len(kinds)] for i in range(n)], dtype=np.float32)


def _masks(B, n, ph, pw, rects, seed):
    """smooth masks whose values cross 0.5 along curves, zero outside each detection's rectangle (what k_assemble_masks leaves)"""
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.randn(B, n, 4, 4, generator=g), (ph, pw), mode="bicubic", align_corners=False)
    m = torch.sigmoid(base * 4 + 0.5).numpy().astype(np.float32)
    ys, xs = np.arange(ph, dtype=np.float32)[:, None], np.arange(pw, dtype=np.float32)[None, :]
    for b in range(B):
        for i in range(n):
            x0, x1, y0, y1 = rects[b, i]
            m[b, i] *= ((xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)).astype(np.float32)
    return m


def _run(lib, masks, flags, rects, H, W, mode, with_rects=True):
    B, n, ph, pw = masks.shape
    d_m, d_f = torch.from_numpy(masks).cuda(), torch.from_numpy(flags).cuda()
    d_r = torch.from_numpy(rects).cuda()
    out = torch.full((B, H, W), 7, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    before = lib.mask_person_window_mode(mode)
    try:
        if with_rects:
            lib.mask_person_mask_rects(st, d_m.data_ptr(), d_f.data_ptr(), d_r.data_ptr(), out.data_ptr(), B, n, ph, pw, H, W)
        else:
            lib.mask_person_mask(st, d_m.data_ptr(), d_f.data_ptr(), out.data_ptr(), B, n, ph, pw, H, W)
        torch.cuda.synchronize()
    finally:
        lib.mask_person_window_mode(before)
    return out.cpu().numpy()


def _flag_rows(n):
    """frames: nothing flagged, one detection, all of them, every other one"""
    f = np.zeros((4, n), dtype=np.uint8)
    f[1, 7 % n] = 1
    f[2] = 1
    f[3, ::2] = 1
    return f


def _case(n, ph, pw, seed):
    flags = _flag_rows(n)
    B = flags.shape[0]
    rects = np.stack([np.roll(_rects(n, ph, pw), b, axis=0) for b in range(B)])
    return _masks(B, n, ph, pw, rects, seed), flags, rects


def _restatement(masks, flags, H, W):
    """the kernel's arithmetic in float32, one operation at a time: PyTorch's source index and weights (align_corners = False), the bilinear
    mix h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d), > 0.5, the count of flagged detections x 255 modulo 256"""
    f32 = np.float32
    B, n, ph, pw = masks.shape

    def axis(inp, out):
        scale = f32(inp) / f32(out)
        src = np.maximum(scale * (np.arange(out, dtype=f32) + f32(0.5)) - f32(0.5), f32(0))
        i0 = src.astype(np.int32)
        i1 = i0 + (i0 < inp - 1)
        l1 = src - i0.astype(f32)
        return i0, i1, l1, f32(1) - l1

    y0, y1, ly, hy = axis(ph, H)
    x0, x1, lx, hx = axis(pw, W)
    out = np.zeros((B, H, W), dtype=np.uint8)
    for b in range(B):
        count = np.zeros((H, W), dtype=np.uint32)
        for i in range(n):
            if not flags[b, i]:
                continue
            m = masks[b, i]
            top = hx[None, :] * m[y0][:, x0] + lx[None, :] * m[y0][:, x1]
            bot = hx[None, :] * m[y1][:, x0] + lx[None, :] * m[y1][:, x1]
            v = hy[:, None] * top + ly[:, None] * bot
            assert v.dtype == np.float32
            count += v > f32(0.5)
        out[b] = ((count * 255) & 0xFF).astype(np.uint8)
    return out


@pytest.mark.parametrize("n", [15, 17], ids=["15_detections", "17_detections"])
@pytest.mark.parametrize("ph,pw,H,W", [(138, 138, 480, 640), (10, 10, 53, 37)], ids=["138_to_640x480", "10_to_37x53"])
def test_windowed_form_equals_the_earlier_form(gpu_lib, ph, pw, H, W, n):
    masks, flags, rects = _case(n, ph, pw, 3)
    old = _run(gpu_lib, masks, flags, rects, H, W, 0)
    new = _run(gpu_lib, masks, flags, rects, H, W, 1)
    rows_only = _run(gpu_lib, masks, flags, rects, H, W, 1, with_rects=False)
    assert new.tobytes() == old.tobytes(), (n, int((new != old).sum()))
    assert rows_only.tobytes() == old.tobytes(), (n, int((rows_only != old).sum()))
    # the case is not trivial: nothing where nothing is flagged, single and overlapping detections elsewhere (2 x 255 wraps to 254)
    assert int(old[0].max()) == 0 and int((old[1] == 255).sum()) > 0 and int((old[2] == 254).sum()) > 0 and 7 not in old


def test_seven_source_rows_occur_at_the_network_size(gpu_lib):
    """(the premise of the derived staging height: 16 output rows of 138 -> 480 touch seven source rows in six of the thirty tile rows, six
    or, at the borders, five in the others)"""
    f32 = np.float32
    scale = f32(138) / f32(480)
    src = np.maximum(scale * (np.arange(480, dtype=f32) + f32(0.5)) - f32(0.5), f32(0)).astype(np.int32)
    rows = [int(min(src[min(t + 15, 479)] + 1, 137) - src[t] + 1) for t in range(0, 480, 16)]
    assert set(rows) == {5, 6, 7} and rows.count(7) == 6


def test_small_case_equals_the_numpy_restatement(gpu_lib):
    masks, flags, rects = _case(15, 8, 8, 9)
    want = _restatement(masks, flags, 27, 20)
    for mode in (0, 1):
        got = _run(gpu_lib, masks, flags, rects, 27, 20, mode)
        assert got.tobytes() == want.tobytes(), (mode, int((got != want).sum()))
    assert int((want == 255).sum()) > 0 and int((want == 0).sum()) > 0


def test_mode_switch_returns_the_previous_value(gpu_lib):
    first = gpu_lib.mask_person_window_mode(-1)
    assert first in (0, 1)
    try:
        assert gpu_lib.mask_person_window_mode(0) == first and gpu_lib.mask_person_window_mode(5) == 0 and gpu_lib.mask_person_window_mode(1) == 0
        assert gpu_lib.mask_person_window_mode(-1) == 1
    finally:
        gpu_lib.mask_person_window_mode(first)
