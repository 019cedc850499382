"""A ResNet stage's first block with its projection shortcut fused into conv3 (amos_mask_conv_chain_device): the fused launch against the
two amos_mask_conv_device launches it replaces, and the backbone with AMOS_MASK_BOTTLENECK_FUSION at 1 against 0 -- bit for bit."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

# (batch, in_h, in_w, cin, planes, cout, stride): the four stages' first blocks at 64 frames per pass
NETWORK_64 = [(64, 138, 138, 64, 64, 256, 1), (64, 138, 138, 256, 128, 512, 2), (64, 69, 69, 512, 256, 1024, 2), (64, 35, 35, 1024, 512, 2048, 2)]
# small odd shapes whose last 128-row tile is partial (run with the 128 x 128 tiles forced: amos_mask_conv_tile_mode(0))
SMALL = [(2, 17, 19, 64, 64, 256, 1), (3, 13, 11, 96, 32, 128, 2), (1, 9, 9, 32, 64, 384, 3), (5, 7, 23, 128, 96, 256, 1)]


def _unfused(lib, x, wd, bd, yc, w3, b3, stride):
    """The two launches the fused one replaces: D = (conv(x, wd) + bd) + 0 to memory, then relu((conv(yc, w3) + b3) + D)."""
    b, cin, h, w = x.shape
    cout, planes = w3.shape[0], yc.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    d = torch.empty((b, cout, yc.shape[2], yc.shape[3]), device="cuda", memory_format=torch.channels_last)
    lib.mask_conv(st, x.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, d.data_ptr(), b, h, w, cin, cout, 1, 1, stride, 0, False)
    y = torch.empty_like(d)
    lib.mask_conv(st, yc.data_ptr(), w3.data_ptr(), b3.data_ptr(), d.data_ptr(), y.data_ptr(), b, yc.shape[2], yc.shape[3], planes, cout, 1, 1, 1, 0, True)
    return y


def _case(lib, shape, seed):
    b, h, w, cin, planes, cout, stride = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    cl = torch.channels_last
    x = torch.randn((b, cin, h, w), device="cuda", generator=g).contiguous(memory_format=cl)
    yc = torch.relu(torch.randn((b, planes, oh, ow), device="cuda", generator=g)).contiguous(memory_format=cl)
    wd = torch.randn((cout, cin, 1, 1), device="cuda", generator=g) / cin ** 0.5
    w3 = torch.randn((cout, planes, 1, 1), device="cuda", generator=g) / planes ** 0.5
    bd = torch.randn(cout, device="cuda", generator=g)
    b3 = torch.randn(cout, device="cuda", generator=g)
    assert lib.mask_conv_chain_supported(b, h, w, cin, planes, cout, stride), shape
    y = torch.full((b, cout, oh, ow), float("nan"), device="cuda").contiguous(memory_format=cl)
    lib.mask_conv_chain(torch.cuda.current_stream().cuda_stream, x.data_ptr(), wd.data_ptr(), bd.data_ptr(), yc.data_ptr(), w3.data_ptr(),
                        b3.data_ptr(), y.data_ptr(), b, h, w, cin, planes, cout, stride)
    ref = _unfused(lib, x, wd, bd, yc, w3, b3, stride)
    torch.cuda.synchronize()
    assert torch.equal(y, ref), (shape, float((y - ref).abs().max()))
    # (zeros of either sign: the ReLU's outputs must match in sign too -- torch.equal does not see it)
    assert torch.equal(torch.signbit(y), torch.signbit(ref)), shape
    assert int((y == 0).sum()) > 0 and int((y > 0).sum()) > 0


@pytest.mark.parametrize("shape", NETWORK_64, ids=lambda s: "x".join(map(str, s)))
def test_fused_shortcut_matches_the_two_launches_at_the_network_shapes(gpu_lib, shape):
    before = gpu_lib.mask_conv_tile_mode(-1)
    try:
        _case(gpu_lib, shape, 1)
    finally:
        gpu_lib.mask_conv_tile_mode(before)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_fused_shortcut_matches_the_two_launches_with_a_partial_tile(gpu_lib, shape):
    before = gpu_lib.mask_conv_tile_mode(0)
    try:
        _case(gpu_lib, shape, 2)
    finally:
        gpu_lib.mask_conv_tile_mode(before)


def test_unsupported_shapes_are_refused(gpu_lib):
    before = gpu_lib.mask_conv_tile_mode(1)  # 128 x 64 tiles: not the kernel's, so not the same bits
    try:
        assert not gpu_lib.mask_conv_chain_supported(64, 138, 138, 64, 64, 256, 1)
        with pytest.raises(gpu_lib.AmosError):
            t = torch.zeros(1 << 20, device="cuda")
            p = t.data_ptr()
            gpu_lib.mask_conv_chain(torch.cuda.current_stream().cuda_stream, p, p, p, p, p, p, p, 1, 8, 8, 64, 64, 256, 1)
    finally:
        gpu_lib.mask_conv_tile_mode(before)
    assert not gpu_lib.mask_conv_chain_supported(64, 138, 138, 64, 64, 192, 1)  # cout % 128
    assert not gpu_lib.mask_conv_chain_supported(64, 138, 138, 48, 64, 256, 1)  # cin % 32


def _trunk_outputs(trunk, x, monkeypatch, switch):
    monkeypatch.setenv("AMOS_MASK_BOTTLENECK_FUSION", switch)
    with torch.no_grad():
        outs = trunk(x)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("frames, fused", [(64, 4), (8, 2)])
def test_trunk_is_bit_identical_with_the_fusion_on_and_off(gpu_lib, monkeypatch, frames, fused):
    """The backbone's four stage outputs with AMOS_MASK_BOTTLENECK_FUSION=1 and =0.  A stage whose two runs with the switch at 0 differ
    (a library convolution that sums in a run-dependent order) is held to that spread instead of to equality."""
    monkeypatch.delenv("AMOS_MASK_CONV1X1", raising=False)
    monkeypatch.delenv("AMOS_GEMM_NARROW", raising=False)
    mask = importlib.import_module("amos_slam_amd.mask")
    eng = mask.MaskEngine(device="cuda:0", seed=0).prepare()
    trunk = eng.net.backbone
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((frames, 3, 550, 550), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    calls = []
    real = gpu_lib.mask_conv_chain
    monkeypatch.setattr(gpu_lib, "mask_conv_chain", lambda *a: (calls.append(a[8:]), real(*a))[1])
    on = _trunk_outputs(trunk, x, monkeypatch, "1")
    assert len(calls) == fused, calls
    off = _trunk_outputs(trunk, x, monkeypatch, "0")
    off2 = _trunk_outputs(trunk, x, monkeypatch, "0")
    assert len(calls) == fused
    for k, (a, b, c) in enumerate(zip(on, off, off2)):
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), k
        if torch.equal(b, c):
            assert torch.equal(a, b), (frames, k, float((a - b).abs().max()))
        else:
            assert float((a - b).abs().max()) <= 2 * float((b - c).abs().max()), (frames, k)
