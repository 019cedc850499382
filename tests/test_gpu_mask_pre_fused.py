"""GPU: the mask pre-processing chain as one kernel (amos_mask_pre_mode 1: k_mask_pre_fused) against the three kernels (mode 0), byte for
byte, for amos_mask_preprocess_batch_device and for the fused-import entry point (whose ORB side must not notice either), and once
against tests/pre_restatement.py directly.  Frame sizes: 640 x 480, an odd one, the smallest the fused import takes, a downscaling one
that still fits the kernel's source window, and 1920 x 1080, which does not and takes the three kernels in both modes."""
import numpy as np
import pytest
import torch

import pre_restatement as pr

pytestmark = pytest.mark.gpu

# (w, h, levels for the extractor, takes the one-pass kernel, bytes of source window: most rows x (most columns x 3, in whole dwords) over
# the 32 x 32 tiles, from the resize geometry: 640 -> 480 -> 640 -> 550 columns, 480 -> 640 -> 480 -> 550 rows at 640 x 480)
SIZES = [(640, 480, 8, True, 32 * 128), (321, 243, 4, True, 17 * 68), (62, 62, 1, True, None), (1280, 720, 8, True, 47 * 248),
         (1920, 1080, 8, False, 70 * 368)]
IDS = [f"{s[0]}x{s[1]}" for s in SIZES]


def _frames(w, h, n, seed):
    """n frames: blocks + noise (corners for FAST at every size); with three, the second is all 0 and the third all 255"""
    rng = np.random.default_rng([w, h, seed])
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        out.append(((90 * ((xx // 16 + yy // 12 + k) % 2))[..., None] + rng.integers(0, 166, (h, w, 3))).astype(np.uint8))
    if n == 3:
        out[1][:], out[2][:] = 0, 255
    out[0][0, 0, 0], out[0][-1, -1, 2] = 0, 255
    return np.stack(out)


def _chain(gpu_lib, pre, d_frames, n, mode):
    before = gpu_lib.mask_pre_mode(mode)
    try:
        out = torch.full((n, 3, 550, 550), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        took = pre.one_pass()[0]
        pre.run(d_frames.data_ptr(), n, out.data_ptr())
        torch.cuda.ExternalStream(pre.stream).synchronize()
        torch.cuda.synchronize()
    finally:
        gpu_lib.mask_pre_mode(before)
    return out.cpu().numpy(), took


def test_mode_switch_returns_the_previous_value(gpu_lib):
    first = gpu_lib.mask_pre_mode(-1)
    assert first in (0, 1)
    assert gpu_lib.mask_pre_mode(0) == first and gpu_lib.mask_pre_mode(5) == 0 and gpu_lib.mask_pre_mode(1) == 0
    assert gpu_lib.mask_pre_mode(first) == 1


@pytest.mark.parametrize("w,h,nl,fits,window", SIZES, ids=IDS)
def test_lds_rule(gpu_lib, w, h, nl, fits, window):
    """Both sides of the rule stated at k_mask_pre_fused: the source window the frame size needs against the kernel's 16 KB."""
    pre = gpu_lib.MaskPreprocessor(w, h, 1)
    before = gpu_lib.mask_pre_mode(1)
    try:
        took, need = pre.one_pass()
        assert took == fits and (need <= 16384) == fits
        assert window is None or need == window
        gpu_lib.mask_pre_mode(0)
        assert pre.one_pass()[0] is False
    finally:
        gpu_lib.mask_pre_mode(before)
    pre.close()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("w,h,nl,fits,window", SIZES, ids=IDS)
def test_one_pass_equals_three_kernels(gpu_lib, w, h, nl, fits, window, n):
    frames = _frames(w, h, n, 40)
    d = torch.from_numpy(frames).cuda()
    pre = gpu_lib.MaskPreprocessor(w, h, n + 1)
    one, took_one = _chain(gpu_lib, pre, d, n, 1)
    three, took_three = _chain(gpu_lib, pre, d, n, 0)
    assert took_one == fits and not took_three
    assert not (one == -7.0).any()
    for f in range(n):
        assert one[f].tobytes() == three[f].tobytes(), f"{w}x{h}, {n} frames: frame {f} differs between the modes"
    again, _ = _chain(gpu_lib, pre, d, n, 1)  # and once more after the three-kernel chain made its buffers
    assert again.tobytes() == one.tobytes()
    pre.close()


def test_one_pass_equals_the_restatement(gpu_lib):
    w, h = 321, 243
    frames = _frames(w, h, 3, 41)
    pre = gpu_lib.MaskPreprocessor(w, h, 3)
    got, took = _chain(gpu_lib, pre, torch.from_numpy(frames).cuda(), 3, 1)
    assert took
    for f in range(3):
        assert got[f].tobytes() == pr.chain(frames[f]).tobytes(), f"frame {f} differs from the restatement"
    pre.close()


def _lay_out(frames, channels, seed):
    """the frames with `channels` bytes per pixel; four: padded rows and frames, an odd first address, noise in every byte that is no pixel's"""
    n, h, w = frames.shape[:3]
    if channels == 3:
        d = torch.from_numpy(frames).cuda()
        return d, d.data_ptr(), h * w * 3, w * 3
    row = w * 4 + 5
    frame = row * h + 7
    flat = np.random.default_rng([seed, 99]).integers(0, 256, 3 + frame * n, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(flat[3:], (n, h, w, 4), (frame, row, 4, 1))[..., :3] = frames
    d = torch.from_numpy(flat).cuda()
    return d, d.data_ptr() + 3, frame, row


@pytest.mark.parametrize("channels,rgb", [(3, False), (4, True)])
@pytest.mark.parametrize("w,h,nl,fits,window", SIZES, ids=IDS)
def test_fused_import_in_both_modes(gpu_lib, w, h, nl, fits, window, channels, rgb):
    """amos_orb_detect_color_with_mask_pre_batch_device: the network input, the keypoints after detect, the descriptors and the padded
    level 0 do not depend on the mode (mode 0: k_import_color_mask + two kernels; mode 1: the plain colour import + the one-pass kernel)."""
    n = 3 if channels == 3 else 1
    frames = _frames(w, h, n, 42 + channels)
    d, ptr, fstride, rstride = _lay_out(frames, channels, 42)
    ext = gpu_lib.OrbExtractor(n_levels=nl, max_width=w, max_height=h, max_batch=n + 1)
    pre = gpu_lib.MaskPreprocessor(w, h, n + 1, stream=ext.stream)
    got = {}
    for mode in (1, 0):
        before = gpu_lib.mask_pre_mode(mode)
        try:
            x = torch.full((n, 3, 550, 550), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert pre.one_pass()[0] == (fits and mode == 1)
            ext.detect_color_with_mask_pre_batch_device(pre, ptr, fstride, rstride, w, h, n, x.data_ptr(), channels=channels, rgb_order=rgb)
            ext.sync()
            levels = [[ext.level_keypoints(l, f).tobytes() for l in range(nl)] for f in range(n)]
            ext.describe_batch_device()
            ext.sync()
            torch.cuda.synchronize()
            got[mode] = (x.cpu().numpy(), levels, [tuple(a.tobytes() for a in ext.batch_fetch(f)) for f in range(n)],
                         [ext.level_image(0, padded=True, frame=f).tobytes() for f in range(n)])
        finally:
            gpu_lib.mask_pre_mode(before)
    assert sum(len(k) for k in got[1][1][0]) > 0
    for f in range(n):
        assert got[1][0][f].tobytes() == got[0][0][f].tobytes(), f"network input of frame {f} differs between the modes"
        assert got[1][1][f] == got[0][1][f], f"keypoints after detect of frame {f} differ between the modes"
        assert got[1][2][f] == got[0][2][f], f"described result of frame {f} differs between the modes"
        assert got[1][3][f] == got[0][3][f], f"padded level 0 of frame {f} differs between the modes"
    if (w, h) == (321, 243):
        for f in range(n):
            assert got[1][0][f].tobytes() == pr.chain(frames[f]).tobytes(), f"frame {f} differs from the restatement"
    pre.close()
    ext.close()
