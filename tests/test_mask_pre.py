"""The mask pass's pre-processing (frame -> the network's [3, 550, 550] input) held to an exact restatement at any frame size.

tests/pre_restatement.py restates the chain in plain numpy with one float32 rounding per operation.  The CPU tests hold that
restatement to the C oracle's 8-bit resize, to the torch chain of mask/pre.py and to the reference's own network input; the GPU tests
hold the three kernels of csrc/amos_mask_pre.hip (MaskPreprocessor.run) and the fused colour import k_import_color_mask
(OrbExtractor.detect_color_with_mask_pre_batch_device) to the restatement BIT FOR BIT: every float operation of the kernels is one
explicitly rounded intrinsic, stage A is integer arithmetic plus a 256-entry table, so there is nothing for a tolerance to absorb.

Sizes (w, h): the smallest and oddest at which taps clamp, weights hit exactly 0.5, or a direction scales by more than 2 either way."""
import importlib
import os
import zlib

import numpy as np
import pytest
import torch

import mask_cases
import pre_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {c: np.load(os.path.join(ROOT, "tests", "golden", f"yolact_{c}.npz")) for c in mask_cases.CASES}
SIZES = [(640, 480), (413, 307), (1241, 376), (200, 700), (960, 1280), (65, 49), (40, 40), (3, 5), (2, 2)]
# fused import: (w, h, the extractor's n_levels); 62 is the smallest side the extractor accepts.  (66, 62): one full 64 x 16 tile plus a 2-column and a
# 14-row remainder, up-scaled 7.3 x 10.3; (129, 81): two tiles plus one column and one row; (1241, 376): down 2.6 x horizontally while up vertically;
# (960, 1280): every weight exactly 0.5
FUSED_SIZES = [(640, 480, 8), (1241, 376, 8), (960, 1280, 8), (129, 81, 2), (66, 62, 1)]


@pytest.fixture(scope="module")
def mask(pkg):
    return importlib.import_module("amos_slam_amd.mask")


# ---- frames, and the restatement of each computed once

def _noise(w, h, seed):
    f = np.random.default_rng([w, h, seed]).integers(0, 256, (h, w, 3), dtype=np.uint8)
    f[0, 0, 0], f[-1, -1, 2] = 0, 255   # both extremes of the 256-entry table, whatever the draw
    return f


def _structured(w, h, seed=0):
    """Flat regions with one vertical and one horizontal step edge; 0 and 255 present (blue is 0 left of the edge and 255 right of it)."""
    f = np.empty((h, w, 3), np.uint8)
    f[:, :w // 2] = (0, 64 + seed, 200)
    f[:, w // 2:] = (255, 10, 90 - seed)
    f[h // 2:, :, 1:] = 255 - f[h // 2:, :, 1:]
    return f


def _frames(w, h, seed):
    """Three frames of one size: two of noise, one structured"""
    return np.stack([_noise(w, h, seed), _noise(w, h, seed + 1), _structured(w, h, seed)])


_CHAIN = {}


def _chain_of(key, frames):
    """pre_restatement.chain of every frame of a batch [n, h, w, 3], computed once per key and never written to"""
    if key not in _CHAIN:
        out = np.stack([pr.chain(f) for f in frames])
        out.setflags(write=False)
        _CHAIN[key] = out
    return _CHAIN[key]


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    if got.tobytes() != want.tobytes():
        raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))   # (records too)
        diff = (raw(got) != raw(want)).any(axis=-1)
        first = np.unravel_index(int(np.argmax(diff)), diff.shape)
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} elements differ, first at {tuple(int(i) for i in first)}: "
                             f"got {got[first]!r}, want {want[first]!r}")


def _case_frame(case="seed0"):
    f = mask_cases.frame(case)
    assert zlib.crc32(f.tobytes()) == int(GOLD[case]["frame_crc"][0]), "the case's frame is not the one the fixture was made from"
    return f


def _engine(mask, device, case="seed0"):
    eng = mask.MaskEngine(device=device, seed=mask_cases.weight_seed(case))
    mask_cases.bias_class_head(eng.net, case)
    return eng


def _iou(a, b):
    union = int((a | b).sum())
    return 1.0 if union == 0 else int((a & b).sum()) / union


# ---- CPU: the restatement itself

@pytest.mark.parametrize("w,h", SIZES)
def test_restated_u8_resize_equals_torch_restatement_and_oracle(mask, ob, w, h):
    """stage_a's integer image against mask.resize_u8_cv (the torch ops the CPU path runs) and, channel by channel, against the C oracle's
    11-bit fixed-point resize: exact.  The float image is the table of it."""
    frame = _noise(w, h, 1)
    v, mid = pr.stage_a(frame)
    assert v.shape == mid.shape == (640, 480, 3) and mid.dtype == np.float32
    assert np.array_equal(v, mask.resize_u8_cv(torch.from_numpy(frame), 480, 640).numpy())
    for c in range(3):
        assert np.array_equal(v[:, :, c], ob.resize_linear_u8(np.ascontiguousarray(frame[:, :, c]), 480, 640)), c
    assert np.array_equal(mid, (v.astype(np.float64) / 255.0).astype(np.float32) * np.float32(255))


@pytest.mark.parametrize("w,h", SIZES)
def test_restated_tap_tables_equal_the_package_rule(mask, w, h):
    """The restatement's scalar tap rule and mask/pre.py's vectorised one are the same tables, clamped ends included."""
    pre = importlib.import_module("amos_slam_amd.mask.pre")
    for src, dst, clamp in ((w, 480, True), (h, 640, False), (480, 640, True), (640, 480, False)):
        for got, want in zip(pr.axis_taps(src, dst, clamp), pre._axis_taps(src, dst, clamp)):
            assert got.tobytes() == want.astype(got.dtype).tobytes(), (src, dst, clamp)


@pytest.mark.parametrize("w,h", SIZES)
def test_restated_chain_against_the_torch_chain_cpu(mask, w, h):
    """chain against cxx_marshalling -> * 255 -> resize_f32_cv -> fast_base_transform on the CPU.  1e-4 is the bound
    test_hip_preprocessing_matches_the_torch_chain uses for the same comparison (torch's bilinear kernel fuses multiply-adds)."""
    frame = _noise(w, h, 2)
    got = pr.chain(frame)
    chw = mask.cxx_marshalling(torch.from_numpy(frame))
    want = mask.fast_base_transform(mask.resize_f32_cv(chw.permute(1, 2, 0) * 255, 640, 480))[0].numpy()
    assert got.shape == want.shape == (3, 550, 550) and got.dtype == np.float32
    err = float(np.abs(got - want).max())
    print(f"{w}x{h}: restatement against the torch chain, max abs difference {err:.3g}")
    assert err < 1e-4, err


@pytest.mark.parametrize("case", list(mask_cases.CASES))
def test_restated_chain_against_the_reference_network_input(case):
    """chain against the tensor the reference's own Python handed to its network (tests/golden, every `sub`-th element), at the bar _run of
    test_mask.py holds the torch chain to."""
    G = GOLD[case]
    got = pr.chain(_case_frame(case)).reshape(-1)[::int(G["sub"][0])]
    print(f"{case}: restatement against the reference's network input, max abs difference {float(np.abs(got - G['batch']).max()):.3g}")
    np.testing.assert_allclose(got, G["batch"], rtol=1e-5, atol=1e-4)


def test_batch_entry_returns_480x640_masks_for_any_frame_size_cpu(mask):
    """eval_image resizes to 640 x 480 whatever came in: eval_bgr_batch gives the [480, 640] mask eval_bgr gives for a 307 x 413 frame."""
    eng = _engine(mask, "cpu")
    frame = np.ascontiguousarray(_case_frame()[:307, :413])
    batch = eng.eval_bgr_batch(torch.from_numpy(frame[None]))
    assert batch.shape == (1, 480, 640) and batch.dtype == torch.uint8
    single = eng.eval_bgr(frame)
    assert single is not None and single.shape == (480, 640)
    assert torch.equal(batch[0], single)


# ---- GPU: the three-kernel chain

def _run_chain(gpu_lib, pre, frames):
    """MaskPreprocessor.run on a tight [n, h, w, 3] batch: the [n, 3, 550, 550] result as numpy"""
    d = torch.from_numpy(frames).cuda()
    out = torch.full((len(frames), 3, 550, 550), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pre.run(d.data_ptr(), len(frames), out.data_ptr())
    torch.cuda.ExternalStream(pre.stream).synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_three_kernel_chain_equals_the_restatement_bit_for_bit(gpu_lib, w, h):
    """amos_mask_preprocess_batch_device on three frames (two of noise, one of flat regions and step edges) with a handle made for five:
    every frame's tensor has the restatement's bits.  A second run of the same handle on other contents gives the restatement of those
    contents (nothing of the first run survives in the intermediate buffers)."""
    pre = gpu_lib.MaskPreprocessor(w, h, 5)
    for seed in (10, 20):
        frames = _frames(w, h, seed)
        assert frames.min() == 0 and frames.max() == 255
        want = _chain_of((w, h, seed), frames)
        got = _run_chain(gpu_lib, pre, frames)
        for f in range(len(frames)):
            _same_bits(got[f], want[f], f"{w}x{h} run with seed {seed}, frame {f}")
    pre.close()


@pytest.mark.gpu
def test_three_kernel_chain_at_and_beyond_its_batch_capacity(gpu_lib):
    w, h = 65, 49
    frames = _frames(w, h, 10)
    pre = gpu_lib.MaskPreprocessor(w, h, 3)
    got = _run_chain(gpu_lib, pre, frames)   # n_frames == max_batch
    want = _chain_of((w, h, 10), frames)
    for f in range(3):
        _same_bits(got[f], want[f], f"full handle, frame {f}")
    d = torch.zeros((4, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((4, 3, 550, 550), dtype=torch.float32, device="cuda")
    with pytest.raises(gpu_lib.AmosError, match="handle made for 3"):
        pre.run(d.data_ptr(), 4, out.data_ptr())
    pre.close()


# ---- GPU: the fused import

def _fused_frames(w, h, seed):
    """Two frames: blocks + noise (corners for FAST at every size) and pure noise"""
    rng = np.random.default_rng([w, h, seed])
    yy, xx = np.mgrid[0:h, 0:w]
    blocks = ((90 * ((xx // 16 + yy // 12) % 2))[..., None] + rng.integers(0, 40, (h, w, 3))).astype(np.uint8)
    return np.stack([blocks, _noise(w, h, seed)])


def _lay_out(frames, layout, seed):
    """The frames in device memory as `layout` asks.  Returns (device buffer, address of frame 0, frame stride, row stride, channels,
    rgb_order, [n, h, w, channels] host view).  "strided4_rgb": four bytes per pixel, rows 5 and frames 7 bytes apart beyond their
    contents, the first pixel 3 bytes into the allocation, every byte between and around the pixels' first three noise."""
    n, h, w = frames.shape[:3]
    if layout == "tight3_bgr":
        d = torch.from_numpy(frames).cuda()
        return d, d.data_ptr(), h * w * 3, w * 3, 3, False, frames
    assert layout == "strided4_rgb"
    row = w * 4 + 5
    frame = row * h + 7
    flat = np.random.default_rng([seed, 99]).integers(0, 256, 3 + frame * n, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[3:], (n, h, w, 4), (frame, row, 4, 1))
    view[..., :3] = frames
    d = torch.from_numpy(flat).cuda()
    return d, d.data_ptr() + 3, frame, row, 4, True, view


def _run_fused(gpu_lib, ext, pre, frames, layout, seed):
    n, h, w = frames.shape[:3]
    d, ptr, fstride, rstride, ch, rgb, view = _lay_out(frames, layout, seed)
    x = torch.full((n, 3, 550, 550), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ext.detect_color_with_mask_pre_batch_device(pre, ptr, fstride, rstride, w, h, n, x.data_ptr(), channels=ch, rgb_order=rgb)
    ext.describe_batch_device()
    ext.sync()
    torch.cuda.synchronize()
    return x.cpu().numpy(), view, rgb


def _check_fused(gpu_lib, ob, ext, x, view, rgb, frames, nl, key, what):
    """Network input == restatement of bytes 0..2 of every pixel (memory order, whatever rgb_order says: the reference hands imRGB to the network
    as it is, the flag only steers cvtColor); keypoints and descriptors == the oracle's on cvtColor's gray."""
    want = _chain_of(key, frames)
    for f in range(len(frames)):
        _same_bits(x[f], want[f], f"{what}: network input of frame {f}")
        ko, do = ob.Oracle(n_levels=nl).extract(ob.color_to_gray(view[f][..., :3], rgb_order=rgb))
        kg, dg = ext.batch_fetch(f)
        _same_bits(kg, ko, f"{what}: keypoints of frame {f}")
        _same_bits(dg, do, f"{what}: descriptors of frame {f}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nl,layout", [s + ("tight3_bgr",) for s in FUSED_SIZES] + [(129, 81, 2, "strided4_rgb"), (640, 480, 8, "strided4_rgb")])
def test_fused_import_equals_the_restatement_and_the_oracle(gpu_lib, ob, w, h, nl, layout):
    """k_import_color_mask + stages B and C: the network input has the restatement's bits and equals the three-kernel chain's; the gray
    side (keypoints, descriptors, the padded level 0 with its reflect-101 border) equals the oracle's.  Handles made for one frame more
    than they are given.  "strided4_rgb": 4 channels in RGB order, padded rows and frames, every source read unaligned."""
    frames = _fused_frames(w, h, 30)
    n = len(frames)
    ext = gpu_lib.OrbExtractor(n_levels=nl, max_width=w, max_height=h, max_batch=n + 1)
    pre = gpu_lib.MaskPreprocessor(w, h, n + 1, stream=ext.stream)
    x, view, rgb = _run_fused(gpu_lib, ext, pre, frames, layout, 30)
    _check_fused(gpu_lib, ob, ext, x, view, rgb, frames, nl, ("fused", w, h, 30), f"{w}x{h} {layout}")
    orc = ob.Oracle(n_levels=nl)
    orc.detect(ob.color_to_gray(view[0][..., :3], rgb_order=rgb))
    _same_bits(ext.level_image(0, padded=True, frame=0), orc.level_image(0, padded=True), f"{w}x{h} {layout}: padded level 0 (reflect-101 border written by the tiles)")
    assert len(ext.batch_fetch(0)[0]) > 0 and len(ext.batch_fetch(1)[0]) > 0
    _same_bits(_run_chain(gpu_lib, pre, frames), x, f"{w}x{h} {layout}: three-kernel chain against the fused import")   # (after the fetches: it reuses the handle's buffers)
    pre.close()
    ext.close()


@pytest.mark.gpu
def test_fused_import_second_call_and_refusals(gpu_lib, ob):
    w, h, nl = 129, 81, 2
    ext = gpu_lib.OrbExtractor(n_levels=nl, max_width=640, max_height=480, max_batch=3)
    pre = gpu_lib.MaskPreprocessor(w, h, 3, stream=ext.stream)
    for seed in (30, 31):   # the second call on the same handles gives the result of the second contents
        frames = _fused_frames(w, h, seed)
        x, view, rgb = _run_fused(gpu_lib, ext, pre, frames, "tight3_bgr", seed)
        _check_fused(gpu_lib, ob, ext, x, view, rgb, frames, nl, ("fused", w, h, seed), f"call with seed {seed}")
    d = torch.zeros((1, 480, 640, 3), dtype=torch.uint8, device="cuda")
    x = torch.zeros((1, 3, 550, 550), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(gpu_lib.AmosError, match="handle made for 129x81 frames, got 128x81"):   # a pre handle made for another size
        ext.detect_color_with_mask_pre_batch_device(pre, d.data_ptr(), 81 * 128 * 3, 128 * 3, 128, 81, 1, x.data_ptr())
    for sw, sh in ((39, 100), (100, 39)):   # a 39-pixel side leaves no room for the two reflected borders
        small = gpu_lib.MaskPreprocessor(sw, sh, 1, stream=ext.stream)
        with pytest.raises(gpu_lib.AmosError, match="too small for the fused import"):
            ext.detect_color_with_mask_pre_batch_device(small, d.data_ptr(), sh * sw * 3, sw * 3, sw, sh, 1, x.data_ptr())
        small.close()
    pre.close()
    ext.close()


# ---- GPU: end to end at a size other than 640 x 480

@pytest.mark.gpu
def test_engine_batch_entry_on_307x413_frames_gpu(mask, gpu_lib):
    """eval_bgr_batch on two 307 x 413 frames: [2, 480, 640] masks that do not depend on which implementation prepared the network's
    input (IoU >= 1 - 1e-3, the bar of the end-to-end assertion at 640 x 480).  The network runs a frame at a time: the convolution
    library has then searched its solvers for these shapes in the one-frame tests of test_mask.py, and two chunks fill the result."""
    eng = _engine(mask, "cuda:0")
    f0 = np.ascontiguousarray(_case_frame()[:307, :413])
    frames = torch.from_numpy(np.stack([f0, np.ascontiguousarray(f0[:, ::-1])])).cuda()
    m_hip = eng.eval_bgr_batch(frames, chunk=1)
    eng.use_hip_pre = False
    m_torch = eng.eval_bgr_batch(frames, chunk=1)
    assert m_hip.shape == m_torch.shape == (2, 480, 640) and m_hip.dtype == torch.uint8
    a, b = (m_hip > 0).cpu().numpy(), (m_torch > 0).cpu().numpy()
    assert a.any(), "the seed0 weights find the person class everywhere: an empty mask compares nothing"
    assert _iou(a, b) >= 1 - 1e-3, _iou(a, b)
