"""GPU box: each stage's first block as ONE launch (amos_mask_conv_chain_device: projection shortcut fused into conv3) against the two
amos_mask_conv_device launches it replaces (shortcut to memory, then conv3 reading it back as its residual), at the network's shapes.
Prints ms per call of both, the saving, the fused launch's TFLOP/s, and whether the outputs are bit-identical.
python tools/bottleneck_fusion_probe.py [frames]"""
import sys
import time

import torch

sys.path.insert(0, ".")
amos = __import__("amos-slam_amd")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
dev = torch.device("cuda:0")
# (name, in_h, cin, planes, cout, stride)
SHAPES = [("layer1 b1 64|64->256", 138, 64, 64, 256, 1), ("layer2 b1 256/2|128->512", 138, 256, 128, 512, 2),
          ("layer3 b1 512/2|256->1024", 69, 512, 256, 1024, 2), ("layer4 b1 1024/2|512->2048", 35, 1024, 512, 2048, 2)]


def timed(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


cl = torch.channels_last
tot = [0.0, 0.0]
for name, H, ci, pl, co, s in SHAPES:
    oh = (H - 1) // s + 1
    x = torch.randn(B, ci, H, H, device=dev).contiguous(memory_format=cl)
    yc = torch.relu(torch.randn(B, pl, oh, oh, device=dev)).contiguous(memory_format=cl)
    wd = torch.randn(co, ci, 1, 1, device=dev) / ci ** 0.5
    w3 = torch.randn(co, pl, 1, 1, device=dev) / pl ** 0.5
    bd, b3 = torch.randn(co, device=dev), torch.randn(co, device=dev)
    d = torch.empty(B, co, oh, oh, device=dev).contiguous(memory_format=cl)
    y0, y1 = torch.empty_like(d), torch.empty_like(d)
    st = torch.cuda.current_stream().cuda_stream
    if not amos.mask_conv_chain_supported(B, H, H, ci, pl, co, s):
        print("%-28s not fused at %d frames" % (name, B))
        continue

    def pair():
        amos.mask_conv(st, x.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, d.data_ptr(), B, H, H, ci, co, 1, 1, s, 0, False)
        amos.mask_conv(st, yc.data_ptr(), w3.data_ptr(), b3.data_ptr(), d.data_ptr(), y0.data_ptr(), B, oh, oh, pl, co, 1, 1, 1, 0, True)

    def fused():
        amos.mask_conv_chain(st, x.data_ptr(), wd.data_ptr(), bd.data_ptr(), yc.data_ptr(), w3.data_ptr(), b3.data_ptr(), y1.data_ptr(), B, H, H, ci, pl, co, s)

    tp, tf = timed(pair), timed(fused)
    tot[0] += tp
    tot[1] += tf
    flop = 2.0 * B * oh * oh * co * (ci + pl)
    print("%-28s pair %.3f ms  fused %.3f ms  saved %.3f ms  fused %.1f TFLOP/s  bit-identical %s"
          % (name, tp, tf, tp - tf, flop / tf / 1e9, bool(torch.equal(y0, y1))))
print("total: pair %.3f ms, fused %.3f ms, saved %.3f ms per pass at %d frames" % (tot[0], tot[1], tot[0] - tot[1], B))
