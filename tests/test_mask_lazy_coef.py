"""Mask coefficients for the displayed detections only: the prediction head's mask layer evaluated at given priors
(amos_mask_coef_at_priors_device), the post-processing chain that takes its coefficients from there
(amos_mask_person_masks_at_priors_device) and the detector's passes that leave the 96 coefficient channels out of the head's output
convolution (AMOS_MASK_LAZY_COEF, default on).

The float32 bound used throughout is derived, not tuned: a dot product of K = 9 x 256 = 2 304 products plus the bias is 2 305 roundings at
most along any summation order (every product is fused into its sum), each relative 2^-24 of a partial sum that never exceeds
S = sum |w x| + |bias|, so |s - s64| <= 2305 x 2^-24 x S before the tanh; the tanh has slope <= 1, and the project allows its tanhf 2 ulp
(tests/test_mask.py, test_fused_head_outputs_equal_the_torch_ops)."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mask_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHORS, DIM, CIN = 3, 32, 256


def _iou(got, want):
    union = int((got | want).sum())
    return 1.0 if union == 0 else int((got & want).sum()) / union


def _golden_person_mask(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"yolact_{case}.npz"))
    return np.unpackbits(g["person_mask_bits"])[:480 * 640].reshape(480, 640).astype(bool)


def _reference(levels, weight, bias, idx):
    """The mask layer at priors idx [B, n] in float64 (direct sums over the zero-padded 3 x 3 patch, tanh in float64).  levels: float32 NCHW
    tensors.  Returns (tanh(s64) [B, n, 32], pre-tanh bound 2305 x 2^-24 x (sum |w x| + |bias|)), zeros for empty slots."""
    w64, b64 = weight.detach().double().cpu(), bias.detach().double().cpu()
    padded = [F.pad(l.detach().double().cpu(), (1, 1, 1, 1)) for l in levels]
    offs = np.cumsum([0] + [l.shape[2] * l.shape[3] * ANCHORS for l in levels])
    B, n = idx.shape
    want, bound = np.zeros((B, n, DIM)), np.zeros((B, n, DIM))
    for b in range(B):
        for s in range(n):
            p = int(idx[b, s])
            if p < 0:
                continue
            l = int(np.searchsorted(offs, p, side="right")) - 1
            cell, a = divmod(p - int(offs[l]), ANCHORS)
            cy, cx = divmod(cell, levels[l].shape[3])
            patch = padded[l][b, :, cy:cy + 3, cx:cx + 3]                     # [cin, 3, 3]: rows cy - 1 .. cy + 1 of the unpadded tensor
            f = w64[a * DIM:(a + 1) * DIM]                                    # [32, cin, 3, 3]
            want[b, s] = torch.tanh((f * patch).sum((1, 2, 3)) + b64[a * DIM:(a + 1) * DIM]).numpy()
            bound[b, s] = (2305 * 2.0 ** -24 * ((f * patch).abs().sum((1, 2, 3)) + b64[a * DIM:(a + 1) * DIM].abs())).numpy()
    return want, bound


def _two_ulp(want):
    return 2 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


def _blocked(x):
    b, c, h, w = x.shape
    return x.view(b, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()   # [b][c / 8][h][w][8]


def _coef_at(gpu_lib, levels, blocked, weight, bias, idx):
    cl = torch.channels_last
    data = [_blocked(l) if f else l.contiguous(memory_format=cl) for l, f in zip(levels, blocked)]
    wl = weight.contiguous(memory_format=cl)
    B, n = idx.shape
    out = torch.full((B, n, DIM), 7.0, device="cuda")
    gpu_lib.mask_coef_at_priors(torch.cuda.current_stream().cuda_stream, [d.data_ptr() for d in data], [tuple(l.shape[2:]) for l in levels], blocked, CIN,
                                wl.data_ptr(), bias.data_ptr(), idx.data_ptr(), B, n, ANCHORS, DIM, out.data_ptr())
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def mask(pkg):
    return importlib.import_module("amos_slam_amd.mask")


@pytest.fixture(scope="module")
def engine(mask, gpu_lib):
    eng = mask.MaskEngine(device="cuda:0", seed=mask_cases.weight_seed("seed0"))
    mask_cases.bias_class_head(eng.net, "seed0")
    return eng.prepare()


@pytest.mark.gpu
def test_coef_at_priors_kernel_against_float64(gpu_lib):
    """The kernel alone: every prior of a small five-level pyramid (every corner, edge and interior cell, every anchor, every level boundary)
    and random priors with empty slots, against the float64 convolution within the derived bound; empty slots zero; level 0 channel-blocked
    gives the bits of level 0 channels-last; a second call gives the same bits."""
    g = torch.Generator().manual_seed(31)
    sizes = ((7, 5), (4, 3), (2, 2), (1, 1), (1, 1))
    levels = [torch.randn(3, CIN, h, w, generator=g).cuda() for h, w in sizes]
    weight, bias = (torch.randn(ANCHORS * DIM, CIN, 3, 3, generator=g) * 0.05).cuda(), torch.randn(ANCHORS * DIM, generator=g).cuda()
    P = sum(h * w for h, w in sizes) * ANCHORS
    assert P == 159
    idx = torch.full((3, P), -1, dtype=torch.int32)
    idx[0] = torch.arange(P, dtype=torch.int32)
    idx[1:, :15] = torch.randint(0, P, (2, 15), generator=g, dtype=torch.int32)
    idx[1, [2, 9]] = -1
    idx[2, [0, 14]] = torch.tensor([-1, -5], dtype=torch.int32)
    want, bound = _reference(levels, weight, bias, idx.numpy())
    # the reference itself against the library's float64 convolution: frame 0 asks for every prior in order
    for l, off in zip(levels, np.cumsum([0] + [h * w * ANCHORS for h, w in sizes])):
        full = torch.tanh(F.conv2d(l[:1].double().cpu(), weight.double().cpu(), bias.double().cpu(), padding=1))   # [1, 96, h, w]
        full = full[0].permute(1, 2, 0).reshape(-1, DIM).numpy()                                                   # [cells x anchors, 32]
        assert np.abs(full - want[0, off:off + full.shape[0]]).max() <= 1e-12
    got = _coef_at(gpu_lib, levels, [False] * 5, weight, bias, idx.cuda())
    err = np.abs(got.double().cpu().numpy() - want)
    limit = bound + _two_ulp(want)
    print("coef_at_priors alone: max error %.3e, max error / bound %.2e" % (err.max(), (err / np.maximum(limit, 1e-300))[idx.numpy() >= 0].max()))
    assert (err <= limit).all()
    empty = (idx < 0).cuda()
    assert int(empty.sum()) == 2 * (P - 15) + 4 and float(got[empty].abs().max()) == 0.0 and float(got[~empty].abs().min()) > 0.0
    assert torch.equal(_coef_at(gpu_lib, levels, [True, False, False, False, False], weight, bias, idx.cuda()), got)
    assert torch.equal(_coef_at(gpu_lib, levels, [False] * 5, weight, bias, idx.cuda()), got)
    with pytest.raises(gpu_lib.AmosError):   # a width the kernel does not take: refused before any launch
        gpu_lib.mask_coef_at_priors(0, [l.data_ptr() for l in levels], [(7, 5)] * 5, [False] * 5, 252, weight.data_ptr(), bias.data_ptr(), idx.data_ptr(), 3, P,
                                    ANCHORS, DIM, got.data_ptr())


def _displayed_priors(mask, pred):
    """The prior index of every displayed detection [B, 15] (-1: empty slot), by the torch-op chain: detect_batch carries a "coefficient"
    tensor that holds the prior's own index, person_mask_batch's selection (the 15 best above the score threshold) follows."""
    det_mod = importlib.import_module("amos_slam_amd.mask.detect")
    post = importlib.import_module("amos_slam_amd.mask.post")
    B, P = pred["loc"].shape[:2]
    tagged = dict(pred)
    tagged["mask"] = torch.arange(P, device="cuda", dtype=torch.float32)[None, :, None].expand(B, P, 1).contiguous()   # exact: P < 2^24
    det = det_mod.detect_batch(tagged)
    valid = det["score"] > post.SCORE_THRESHOLD
    top, order = torch.where(valid, det["score"], torch.full_like(det["score"], -1.0)).topk(post.TOP_K_DISPLAY, dim=1)
    prior = torch.gather(det["mask"][..., 0], 1, order).to(torch.int32)
    return torch.where(top > post.SCORE_THRESHOLD, prior, torch.full_like(prior, -1))


@pytest.mark.gpu
def test_coef_at_priors_against_the_full_head(mask, gpu_lib, engine):
    """On the network's own upfeature tensors (weight set seed0, two golden frames): the displayed detections' coefficients from the full
    "mask" tensor (Winograd / library convolution of all 19 248 priors) and from the new kernel, each against the float64 convolution of the
    same upfeature tensor.  The new kernel within the derived bound; the two within that bound plus the full path's own measured error.
    Measured on MI355X (30 displayed priors; DESIGN.md section 7, "Lazy mask coefficients"): |new - f64| <= 5.4e-9, |full - f64| <= 1.7e-8,
    |new - full| <= 1.7e-8, the bound <= 2.8e-5."""
    frames = torch.from_numpy(np.stack([mask_cases.frame(c) for c in ("seed0", "ref122_w0")])).cuda()
    with torch.no_grad():
        x = engine._preprocess_hip(frames)
        full = engine._forward(x)
        engine.net.lazy_coef = True
        try:
            lazy = engine._forward(x)
        finally:
            engine.net.lazy_coef = False
    torch.cuda.synchronize()
    assert full["mask"].shape == (2, 19248, DIM) and "mask" not in lazy and len(lazy["upfeature"]) == 5
    idx = _displayed_priors(mask, full)
    assert int((idx >= 0).sum()) >= 2, "no displayed detection: the comparison would be empty"
    ups = lazy["upfeature"]
    assert all(torch.is_tensor(u) and u.shape[:2] == (2, CIN) for u in ups)   # (two frames: no channel-blocked level)
    layer = lazy["mask_layer"]
    want, bound = _reference(ups, layer.weight, layer.bias, idx.cpu().numpy())
    new = _coef_at(gpu_lib, ups, [False] * 5, layer.weight.detach(), layer.bias.detach(), idx).double().cpu().numpy()
    sel = idx.clamp(min=0).long()[..., None].expand(-1, -1, DIM)
    old = torch.where((idx >= 0)[..., None], torch.gather(full["mask"], 1, sel), torch.zeros((), device="cuda")).double().cpu().numpy()
    e_new, e_full = np.abs(new - want), np.abs(old - want)
    print("displayed priors %d: |new - f64| max %.3e, |full - f64| max %.3e, |new - full| max %.3e, bound max %.3e"
          % (int((idx >= 0).sum()), e_new.max(), e_full.max(), np.abs(new - old).max(), (bound + _two_ulp(want)).max()))
    assert (e_new <= bound + _two_ulp(want)).all()
    assert (np.abs(new - old) <= bound + _two_ulp(want) + e_full).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames", [2, 8])
def test_lazy_pass_gives_the_masks_of_the_full_pass(mask, gpu_lib, engine, monkeypatch, n_frames):
    """eval_net_input_batch with AMOS_MASK_LAZY_COEF on (the default) and off: the same `found`, person masks at IoU >= 1 - 1e-3 of each other
    and of the golden masks.  Two frames: a small pass (side streams, every level channels-last); eight: the smallest pass whose level 0
    travels channel-blocked through the head."""
    cases = (["seed0", "ref122_w0", "tum_w0"] * 3)[:n_frames]
    frames = torch.from_numpy(np.stack([mask_cases.frame(c) for c in cases])).cuda()
    calls = []
    real = gpu_lib.mask_person_masks_at_priors
    monkeypatch.setattr(gpu_lib, "mask_person_masks_at_priors", lambda *a: (calls.append(a[6]), real(*a))[1])   # (the levels' blocked flags)
    got = {}
    with torch.no_grad():
        x = engine._preprocess_hip(frames)
        for mode in ("1", "0"):
            monkeypatch.setenv("AMOS_MASK_LAZY_COEF", mode)
            del calls[:]
            masks = engine.eval_net_input_batch(x).clone()
            again, found = engine._masks_of(x, 640, 480)
            torch.cuda.synchronize()
            assert torch.equal(masks, again)
            assert calls == ([[n_frames >= 8, False, False, False, False]] * 2 if mode == "1" else [])
            got[mode] = (masks.cpu().numpy() > 0, found.cpu().numpy())
    assert np.array_equal(got["1"][1], got["0"][1]) and got["1"][1].all()
    assert sum(int(m.sum()) for m in got["1"][0]) > 0
    for k, case in enumerate(cases):
        iou_modes, iou_gold = _iou(got["1"][0][k], got["0"][0][k]), _iou(got["1"][0][k], _golden_person_mask(case))
        print("frame %d (%s): IoU lazy / full %.6f, lazy / golden %.6f, %d mask pixels" % (k, case, iou_modes, iou_gold, int(got["1"][0][k].sum())))
        assert iou_modes >= 1 - 1e-3 and iou_gold >= 1 - 1e-3, (k, case)
