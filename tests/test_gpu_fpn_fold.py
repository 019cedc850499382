"""The feature pyramid's top-down resize inside the lateral convolution (amos_mask_conv_upsampled_residual_device,
k_conv_gemm<.., false, false, true>): the one launch against amos_mask_bilinear_nhwc_device followed by amos_mask_conv_device with the
resized tensor as its residual, and the network's pyramid with amos_mask_fpn_fold_mode at 1 against 0 -- byte for byte."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

CHANNELS = [(32, 64), (64, 128)]            # the smallest sizes amos_mask_conv_supported admits (64: 128 x 64 tiles whatever the mode)
BATCHES = [2, 3]
# coarse -> fine: odd ratios like the network's 18 -> 35 and 35 -> 69; M = batch x fine pixels is no multiple of 128, so tiles cross frame
# borders and the last one is partial
SIZES = [((3, 3), (5, 5)), ((5, 5), (9, 9)), ((4, 5), (7, 9))]


def _scale(coarse, fine):
    """PyTorch's area_pixel_compute_scale for a given output size, in float32"""
    return float(torch.tensor(coarse, dtype=torch.float32) / fine)


def _one(lib, cin, cout, batch, coarse, fine, relu, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    cl = torch.channels_last
    (uh, uw), (h, w) = coarse, fine
    x = torch.randn((batch, cin, h, w), device="cuda", generator=g).contiguous(memory_format=cl)
    top = torch.randn((batch, cout, uh, uw), device="cuda", generator=g).contiguous(memory_format=cl)
    wt = torch.randn((cout, cin, 1, 1), device="cuda", generator=g) / cin ** 0.5
    bias = torch.randn(cout, device="cuda", generator=g)
    sh, sw = _scale(uh, h), _scale(uw, w)
    st = torch.cuda.current_stream().cuda_stream
    up = torch.empty((batch, cout, h, w), device="cuda").contiguous(memory_format=cl)
    lib.mask_bilinear_nhwc(st, top.data_ptr(), up.data_ptr(), batch, uh, uw, h, w, cout, sh, sw)
    want = torch.empty_like(up)
    lib.mask_conv(st, x.data_ptr(), wt.data_ptr(), bias.data_ptr(), up.data_ptr(), want.data_ptr(), batch, h, w, cin, cout, 1, 1, 1, 0, relu)
    got = torch.full((batch, cout, h, w), float("nan"), device="cuda").contiguous(memory_format=cl)
    lib.mask_conv_upsampled_residual(st, x.data_ptr(), wt.data_ptr(), bias.data_ptr(), top.data_ptr(), got.data_ptr(), batch, h, w, cin, cout, uh, uw, sh, sw,
                                     relu)
    torch.cuda.synchronize()
    case = (cin, cout, batch, coarse, fine, relu)
    assert got.permute(0, 2, 3, 1).contiguous().cpu().numpy().tobytes() == want.permute(0, 2, 3, 1).contiguous().cpu().numpy().tobytes(), case
    assert bool(torch.isfinite(got).all()), case
    if relu:
        assert int((got == 0).sum()) > 0 and int((got > 0).sum()) > 0, case


@pytest.mark.parametrize("tile_mode", [0, 1], ids=["wide", "narrow"])
@pytest.mark.parametrize("cin,cout", CHANNELS, ids=lambda v: str(v))
def test_fused_resize_matches_the_two_launches(gpu_lib, cin, cout, tile_mode):
    before = gpu_lib.mask_conv_tile_mode(tile_mode)
    try:
        seed = 0
        for batch in BATCHES:
            for coarse, fine in SIZES:
                for relu in (False, True):
                    seed += 1
                    _one(gpu_lib, cin, cout, batch, coarse, fine, relu, seed)
    finally:
        gpu_lib.mask_conv_tile_mode(before)


def test_mode_switch_returns_the_previous_value(gpu_lib):
    first = gpu_lib.mask_fpn_fold_mode(-1)
    assert first in (0, 1)
    try:
        assert gpu_lib.mask_fpn_fold_mode(0) == first and gpu_lib.mask_fpn_fold_mode(5) == 0 and gpu_lib.mask_fpn_fold_mode(1) == 0
        assert gpu_lib.mask_fpn_fold_mode(-1) == 1
    finally:
        gpu_lib.mask_fpn_fold_mode(first)


def test_invalid_arguments_are_refused(gpu_lib):
    t = torch.zeros(1 << 16, device="cuda")
    p, st = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    for args in ((p, p, p, None, p, 1, 5, 5, 32, 64, 3, 3, 0.6, 0.6, False),      # no coarser tensor
                 (p, p, p, p, p, 1, 5, 5, 48, 64, 3, 3, 0.6, 0.6, False),         # cin % 32
                 (p, p, p, p, p, 1, 5, 5, 32, 64, 0, 3, 0.6, 0.6, False),         # empty coarser level
                 (p, p, p, p + 4, p, 1, 5, 5, 32, 64, 3, 3, 0.6, 0.6, False)):    # alignment
        with pytest.raises(gpu_lib.AmosError):
            gpu_lib.mask_conv_upsampled_residual(st, *args)


def _pyramid(gpu_lib, net, fpn, feats, monkeypatch, mode):
    """the pyramid's five outputs and, in the order they are made (deepest first), its three merged levels, with amos_mask_fpn_fold_mode at `mode`"""
    merged = []
    real = net.lateral_conv
    monkeypatch.setattr(net, "lateral_conv", lambda *a: (merged.append(real(*a)), merged[-1])[1])
    before = gpu_lib.mask_fpn_fold_mode(mode)
    try:
        with torch.no_grad():
            outs = [t.clone() for t in fpn(feats)]
        torch.cuda.synchronize()
    finally:
        gpu_lib.mask_fpn_fold_mode(before)
        monkeypatch.setattr(net, "lateral_conv", real)
    assert len(outs) == 5 and len(merged) == 3
    return outs, merged


def _bytes(t):
    return t.contiguous().cpu().numpy().tobytes()


@pytest.mark.parametrize("forced", [False, True], ids=["automatic_rule", "every_1x1_on_the_gemm"])
@pytest.mark.parametrize("frames", [1, 2])
def test_pyramid_is_bit_identical_with_the_fold_on_and_off(gpu_lib, monkeypatch, frames, forced):
    """YolactR50's pyramid on the backbone's three feature shapes with amos_mask_fpn_fold_mode at 1 and at 0.
    Automatic rule: at one and two frames only the 512 -> 256 lateral at 69 x 69 runs on the GEMM and takes the fused entry; the 1024 -> 256
    lateral at 35 x 35 has too few work-groups for it and keeps its two launches in both modes.  With AMOS_MASK_CONV1X1=1 all three laterals
    run on the GEMM and both that have a level above them take the fused entry.
    The library convolutions that run at these sizes (the deeper laterals under the automatic rule, the small 3 x 3 layers) sum in a
    run-dependent order on this hardware: two runs with the switch at 0 differ in every level (measured: up to 2e-6).  So a tensor is
    held to EQUAL BYTES wherever two runs with the switch at 0 give equal bytes -- with the 1 x 1 layers forced onto the GEMM that is every
    merged level, asserted -- and to twice that run-to-run spread where they do not."""
    for name in ("AMOS_MASK_CONV1X1", "AMOS_GEMM_NARROW", "AMOS_MASK_FPN_FOLD"):
        monkeypatch.delenv(name, raising=False)
    if forced:
        monkeypatch.setenv("AMOS_MASK_CONV1X1", "1")
    mask = importlib.import_module("amos_slam_amd.mask")
    net = importlib.import_module("amos_slam_amd.mask.net")
    eng = mask.MaskEngine(device="cuda:0", seed=0).prepare()
    fpn = eng.net.fpn
    g = torch.Generator(device="cuda").manual_seed(5)
    cl = torch.channels_last
    feats = [torch.relu(torch.randn((frames, c, s, s), device="cuda", generator=g)).contiguous(memory_format=cl) for c, s in ((512, 69), (1024, 35), (2048, 18))]
    calls = []
    real = gpu_lib.mask_conv_upsampled_residual
    monkeypatch.setattr(gpu_lib, "mask_conv_upsampled_residual", lambda *a: (calls.append(a[6:13]), real(*a))[1])
    on = _pyramid(gpu_lib, net, fpn, feats, monkeypatch, 1)
    want_calls = [(frames, 35, 35, 1024, 256, 18, 18)] if forced else []
    want_calls.append((frames, 69, 69, 512, 256, 35, 35))
    assert calls == want_calls, calls
    off = _pyramid(gpu_lib, net, fpn, feats, monkeypatch, 0)
    off2 = _pyramid(gpu_lib, net, fpn, feats, monkeypatch, 0)
    assert calls == want_calls
    for kind in (1, 0):  # the merged levels (deepest first), then the outputs
        for k, (a, b, c) in enumerate(zip(on[kind], off[kind], off2[kind])):
            assert a.shape == b.shape and bool(torch.isfinite(a).all()), (kind, k)
            stable = _bytes(b) == _bytes(c)
            if forced and kind == 1:
                assert stable, (frames, k)  # this project's GEMM alone: the same bits every run
            if stable:
                assert _bytes(a) == _bytes(b), (frames, kind, k, float((a - b).abs().max()))
            else:
                assert float((a - b).abs().max()) <= 2 * float((b - c).abs().max()), (frames, kind, k)


@pytest.mark.parametrize("frames", [1, 2, 64])
def test_laterals_are_bit_identical_on_the_same_level_above(gpu_lib, monkeypatch, frames):
    """Each lateral of YolactR50's pyramid that has a level above it, at the network's sizes, with the SAME tensor above on both sides (so no
    library convolution's run-dependent sum comes between): lateral_conv with the switch at 1 and at 0, equal bytes.  At 64 frames -- a
    lane's pass -- both run on the GEMM under the automatic rule and take the fused entry with 128 x 128 tiles."""
    for name in ("AMOS_MASK_CONV1X1", "AMOS_GEMM_NARROW", "AMOS_MASK_FPN_FOLD"):
        monkeypatch.delenv(name, raising=False)
    mask = importlib.import_module("amos_slam_amd.mask")
    net = importlib.import_module("amos_slam_amd.mask.net")
    fpn = mask.MaskEngine(device="cuda:0", seed=0).prepare().net.fpn
    g = torch.Generator(device="cuda").manual_seed(6)
    cl = torch.channels_last
    folded = 0
    for lat, (cin, s), above in ((fpn.lat_layers[1], (1024, 35), 18), (fpn.lat_layers[2], (512, 69), 35)):
        x = torch.relu(torch.randn((frames, cin, s, s), device="cuda", generator=g)).contiguous(memory_format=cl)
        top = torch.randn((frames, 256, above, above), device="cuda", generator=g).contiguous(memory_format=cl)
        before = gpu_lib.mask_fpn_fold_mode(1)
        try:
            with torch.no_grad():
                fold = net.lateral_fold(lat, x, top)
                a = net.lateral_conv(lat, x, top)
                gpu_lib.mask_fpn_fold_mode(0)
                assert not net.lateral_fold(lat, x, top)
                b = net.lateral_conv(lat, x, top)
            torch.cuda.synchronize()
        finally:
            gpu_lib.mask_fpn_fold_mode(before)
        folded += int(fold)
        if fold:
            assert _bytes(a) == _bytes(b), (frames, cin, float((a - b).abs().max()))
    assert folded == (2 if frames == 64 else 1)
