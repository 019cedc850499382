"""tests/pre_restatement.py -- the mask pass's pre-processing chain restated in plain numpy, one float32
rounding per operation and nothing fused:

  stage_a  yolact::evalImage (yolact.cc:220, 385-451): cv::resize(BGR u8 -> W480 x H640) [sic, swapped], u8 / 255.0 as float, and
           eval_image's "* 255" (yolact_interface.py:862-864)
  stage_b  eval_image's cv2.resize(float32, (640, 480)) (yolact_interface.py:865)
  stage_c  FastBaseTransform (utils/augmentations.py:616-657): bilinear to 550 x 550 (align_corners=False), (x - MEANS) / STD in BGR
           order, planes reversed to RGB

TEST INFRASTRUCTURE ONLY: tests/test_mask_pre.py holds the three kernels of csrc/amos_mask_pre.hip and the fused import
k_import_color_mask (csrc/orb_kernels.h) to it bit for bit, and holds it in turn to the C oracle's 8-bit resize, to the torch chain of
mask/pre.py and to the reference's own network input (tests/golden/yolact_*.npz).  No torch in here: every float array is np.float32 and
every product, sum, difference and quotient is a separate numpy operation, which rounds once, like the kernels' __fmul_rn / __fadd_rn /
__fsub_rn / __fdiv_rn."""
import numpy as np

f32 = np.float32
MID_W, MID_H = 480, 640      # yolact.cc:220  cv::Size(480, 640)
BACK_W, BACK_H = 640, 480    # yolact_interface.py:865
NET = 550                    # cfg.max_size
MEANS = (103.94, 116.78, 123.68)  # BGR, data/config.py:28-29
STD = (57.38, 57.12, 58.40)


def axis_taps(src_n, dst_n, clamp_fraction):
    """cv::resize INTER_LINEAR: (first tap, second tap, fraction) per destination index.  The source coordinate is computed in double and
    rounded to float32; the horizontal pass resets the fraction to 0 at both clamped ends, the vertical pass only clips the indices."""
    scale = 1.0 / (float(dst_n) / float(src_n))
    s0, s1, fr = np.zeros(dst_n, np.int64), np.zeros(dst_n, np.int64), np.zeros(dst_n, f32)
    for d in range(dst_n):
        fx = f32((d + 0.5) * scale - 0.5)
        s = int(np.floor(fx))
        fx = f32(fx - f32(s))
        if clamp_fraction:
            if s < 0:
                fx, s = f32(0), 0
            if s >= src_n - 1:
                fx, s = f32(0), src_n - 1
        s0[d], s1[d], fr[d] = min(max(s, 0), src_n - 1), min(max(s + 1, 0), src_n - 1), fx
    return s0, s1, fr


def _fixed(f):
    """11-bit fixed-point weights of the 8-bit resize: products in float32, rounded half to even."""
    a1 = np.rint(f * f32(2048)).astype(np.int64)
    a0 = np.rint((f32(1) - f) * f32(2048)).astype(np.int64)
    return a0, a1


def stage_a(bgr):
    """bgr uint8 [H, W, 3] -> (v int64 [640, 480, 3], the 8-bit resize's result; mid float32 [640, 480, 3] = float(double(v) / 255.0) * 255.0f)"""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    h, w = bgr.shape[:2]
    x0, x1, fx = axis_taps(w, MID_W, True)
    y0, y1, fy = axis_taps(h, MID_H, False)
    a0, a1 = (t[None, :, None] for t in _fixed(fx))
    b0, b1 = (t[:, None, None] for t in _fixed(fy))
    p = bgr.astype(np.int64)
    r0, r1 = p[y0], p[y1]                                  # [640, W, 3]
    h0 = r0[:, x0] * a0 + r0[:, x1] * a1                   # [640, 480, 3]
    h1 = r1[:, x0] * a0 + r1[:, x1] * a1
    v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
    assert v.min() >= 0 and v.max() <= 255
    lut = (np.arange(256, dtype=np.float64) / 255.0).astype(f32) * f32(255)
    return v, lut[v]


def stage_b(mid):
    """mid float32 [640, 480, 3] -> back float32 [480, 640, 3]: float cv::resize, horizontal then vertical, weights 1.0f - f and f"""
    assert mid.dtype == f32 and mid.shape == (MID_H, MID_W, 3)
    x0, x1, fx = axis_taps(MID_W, BACK_W, True)
    y0, y1, fy = axis_taps(MID_H, BACK_H, False)
    fx0, fx1 = (f32(1) - fx)[None, :, None], fx[None, :, None]
    fy0, fy1 = (f32(1) - fy)[:, None, None], fy[:, None, None]
    r0, r1 = mid[y0], mid[y1]                              # [480, 480, 3]
    h0 = r0[:, x0] * fx0 + r0[:, x1] * fx1                 # [480, 640, 3]
    h1 = r1[:, x0] * fx0 + r1[:, x1] * fx1
    out = h0 * fy0 + h1 * fy1
    assert out.dtype == f32
    return out


def _torch_axis(in_n, out_n):
    """PyTorch's area_pixel_compute_source_index (align_corners=False) in float32: (index, second index, weight of the first, of the second)"""
    scale = f32(in_n) / f32(out_n)
    i = np.arange(out_n, dtype=f32)
    r = np.maximum(scale * (i + f32(0.5)) - f32(0.5), f32(0))
    i0 = r.astype(np.int64)                                # r >= 0: truncation is the floor
    i1 = i0 + (i0 < in_n - 1)
    l1 = r - i0.astype(f32)
    l0 = f32(1) - l1
    assert r.dtype == l1.dtype == l0.dtype == f32
    return i0, i1, l0, l1


def stage_c(back):
    """back float32 [480, 640, 3] (BGR, 0..255) -> float32 [3, 550, 550], normalised, planes in RGB order"""
    assert back.dtype == f32 and back.shape == (BACK_H, BACK_W, 3)
    h0, h1, hl0, hl1 = _torch_axis(BACK_H, NET)
    w0, w1, wl0, wl1 = _torch_axis(BACK_W, NET)
    wl0, wl1 = wl0[None, :, None], wl1[None, :, None]
    hl0, hl1 = hl0[:, None, None], hl1[:, None, None]
    ra, rb = back[h0], back[h1]                            # [550, 640, 3]
    top = wl0 * ra[:, w0] + wl1 * ra[:, w1]                # [550, 550, 3]
    bot = wl0 * rb[:, w0] + wl1 * rb[:, w1]
    v = hl0 * top + hl1 * bot
    out = (v - np.array(MEANS, f32)) / np.array(STD, f32)
    assert out.dtype == f32
    return np.ascontiguousarray(out.transpose(2, 0, 1)[::-1])


def chain(bgr):
    """uint8 [H, W, 3] frame (the three bytes of a pixel in memory order) -> the network's float32 [3, 550, 550] input"""
    return stage_c(stage_b(stage_a(bgr)[1]))
