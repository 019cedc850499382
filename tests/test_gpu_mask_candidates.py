"""Fast-NMS candidates from compact lists above the display score (AMOS_MASK_CANDIDATES, default on): the head's kernel appends every class
score above post.SCORE_THRESHOLD to the list of its (frame, class) instead of writing a softmax or class-score tensor
(amos_mask_head_candidates_device), top-k runs over the lists (amos_mask_topk_lists_device), Fast NMS skips the empty ones, and the rest of the
post-processing is the dense path's (amos_mask_person_masks_candidates[_at_priors]_device).

Everything here is compared bit for bit: a score at or under the threshold is never displayed, suppresses only lower scores of its class, and
sorts behind every score above the threshold (ties by index), so leaving it out changes neither the displayed set nor its order.  The one
comparison with a tolerance is the one against the torch-op chain, which carries the tolerance of the existing fused test (the 32-term
prototype sums are rounded in another order there)."""
import importlib

import numpy as np
import pytest
import torch

import mask_cases

ANCHORS, C1, DIM, CIN = 3, 81, 32, 8
K, K_LIST = 200, 1024          # AMOS_MASK_NMS_TOP_K; kTopkList of amos_mask_post.hip (lists up to it are sorted in LDS, longer ones selected)
PH = PW = 32                   # prototype grid of the synthetic heads
OUT_H, OUT_W = 96, 128


@pytest.fixture(scope="module")
def mask(pkg):
    return importlib.import_module("amos_slam_amd.mask")


@pytest.fixture(scope="module")
def engine(mask, gpu_lib):
    eng = mask.MaskEngine(device="cuda:0", seed=mask_cases.weight_seed("seed0"))
    mask_cases.bias_class_head(eng.net, "seed0")
    return eng.prepare()


def _iou(got, want):
    union = int((got | want).sum())
    return 1.0 if union == 0 else int((got & want).sum()) / union


class _Head:
    """A synthetic prediction head: the raw output tensors of `sizes` levels (channels [12 box | 243 class | 96 coefficient | pad] = 384, or
    without the coefficients = 256), priors, prototypes, and for the lazy entries upfeature levels and a mask layer of 8 input channels."""

    def __init__(self, sizes, batch, seed):
        g = torch.Generator().manual_seed(seed)
        net = importlib.import_module("amos_slam_amd.mask.net")
        self.sizes, self.B = sizes, batch
        self.P = sum(h * w for h, w in sizes) * ANCHORS
        self.logits = [torch.randn(batch, h * w, ANCHORS, C1, generator=g) * 3 for h, w in sizes]
        for l in self.logits:
            l[..., 1] += 2.0   # (persons among the displayed detections)
        self.box = [torch.randn(batch, h * w, ANCHORS * 4, generator=g) * 0.5 for h, w in sizes]
        self.coef_raw = [torch.randn(batch, h * w, ANCHORS * DIM, generator=g) for h, w in sizes]
        self.bias = torch.randn(384, generator=g) * 0.01
        self.priors = net.build_priors(sizes, "cuda")
        self.proto = torch.relu(torch.randn(batch, PH, PW, DIM, generator=g)).cuda()
        self.ups = [torch.randn(batch, CIN, h, w, generator=g).cuda().contiguous(memory_format=torch.channels_last) for h, w in sizes]
        self.weight = (torch.randn(ANCHORS * DIM, CIN, 3, 3, generator=g) * 0.3).cuda().contiguous(memory_format=torch.channels_last)
        self.mask_bias = torch.randn(ANCHORS * DIM, generator=g).cuda()

    def raw(self, level, with_coef):
        b, cells = self.logits[level].shape[:2]
        parts = [self.box[level], self.logits[level].reshape(b, cells, -1)] + ([self.coef_raw[level]] if with_coef else [])
        r = torch.cat(parts, -1)
        return torch.cat((r, torch.zeros(b, cells, (384 if with_coef else 256) - r.shape[-1])), -1).contiguous().cuda()

    def head(self, gpu_lib, with_coef, candidates):
        """The head's kernel over every level: (loc, conf or None, coef or None, candidate buffer or None)"""
        st = torch.cuda.current_stream().cuda_stream
        B, P = self.B, self.P
        loc = torch.zeros(B, P, 4, device="cuda")
        conf = None if candidates else torch.zeros(B, P, C1, device="cuda")
        coef = torch.zeros(B, P, DIM, device="cuda") if with_coef else None
        cand = None
        bias = self.bias[:384 if with_coef else 256].contiguous().cuda()
        if not with_coef:
            bias[255:] = 0
        if candidates:
            cand = torch.full((gpu_lib.mask_candidates_bytes(B, P, C1),), 0xA5, dtype=torch.uint8, device="cuda")   # (stale bytes everywhere)
            gpu_lib.mask_candidates_reset(st, cand.data_ptr(), B, C1)
        off = 0
        for i, (h, w) in enumerate(self.sizes):
            raw = self.raw(i, with_coef)
            if candidates:
                gpu_lib.mask_head_candidates(st, raw.data_ptr(), bias.data_ptr(), loc.data_ptr(), coef.data_ptr() if with_coef else None, cand.data_ptr(),
                                             0.15, B, h * w, raw.shape[-1], ANCHORS, C1, DIM, P, off)
            else:
                gpu_lib.mask_head_outputs_scores(st, raw.data_ptr(), bias.data_ptr(), loc.data_ptr(), conf.data_ptr(), coef.data_ptr() if with_coef else None,
                                                 None, 0.05, B, h * w, raw.shape[-1], ANCHORS, C1, DIM, P, off)
            off += h * w * ANCHORS
        torch.cuda.synchronize()
        return loc, conf, coef, cand

    def post(self, gpu_lib, loc, scores, coef, candidates):
        """masks, found of the fused post-processing: from a coefficient tensor, or (coef None) the lazy form over the upfeature levels"""
        st = torch.cuda.current_stream().cuda_stream
        B, P = self.B, self.P
        n = gpu_lib.mask_post_workspace_bytes(B, P, C1, DIM, PH, PW)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        out = torch.full((B, OUT_H, OUT_W), 7, dtype=torch.uint8, device="cuda")
        found = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
        tail = (self.priors.data_ptr(), self.proto.data_ptr(), B, P, C1, DIM, PH, PW, OUT_H, OUT_W, ws.data_ptr(), n, out.data_ptr(), found.data_ptr())
        if coef is not None:
            (gpu_lib.mask_person_masks_candidates if candidates else gpu_lib.mask_person_masks)(st, loc.data_ptr(), scores.data_ptr(), coef.data_ptr(), *tail)
        else:
            gpu_lib.mask_person_masks_at_priors(st, loc.data_ptr(), scores.data_ptr(), "candidates" if candidates else False, [u.data_ptr() for u in self.ups],
                                                list(self.sizes), [False] * len(self.sizes), CIN, ANCHORS, self.weight.data_ptr(), self.mask_bias.data_ptr(), *tail)
        torch.cuda.synchronize()
        return out, found

    def compare(self, gpu_lib, torch_too=False):
        """Both forms of the head and of the post-processing, dense against lists: bit for bit.  Returns (conf, masks, found) of the dense path."""
        result = None
        for with_coef in (True, False):
            loc, conf, coef, _ = self.head(gpu_lib, with_coef, False)
            loc2, _, coef2, cand = self.head(gpu_lib, with_coef, True)
            assert torch.equal(loc, loc2) and (not with_coef or torch.equal(coef, coef2))
            want = self.post(gpu_lib, loc, conf, coef, False)
            got = self.post(gpu_lib, loc2, cand, coef2, True)
            loc3, _, coef3, cand3 = self.head(gpu_lib, with_coef, True)   # (a second run: the lists may come in another order)
            again = self.post(gpu_lib, loc3, cand3, coef3, True)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), with_coef
            assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), with_coef
            assert set(want[1].cpu().tolist()) <= {0, 1}
            if with_coef:
                result = (conf, want[0], want[1])
                if torch_too:
                    post = importlib.import_module("amos_slam_amd.mask.post")
                    det = importlib.import_module("amos_slam_amd.mask.detect")
                    tm, tf = post.person_mask_batch(det.detect_batch({"loc": loc, "conf": conf, "mask": coef, "priors": self.priors, "proto": self.proto}), OUT_W, OUT_H)
                    torch.cuda.synchronize()
                    assert torch.equal(tf, got[1].bool())
                    for b in range(self.B):   # (the tolerance of test_fused_post_processing_equals_the_torch_ops_path)
                        assert int((tm[b] != got[0][b]).sum()) <= 40 and _iou((tm[b] > 0).cpu().numpy(), (got[0][b] > 0).cpu().numpy()) >= 1 - 1e-3, b
        return result

    def row_counts(self, conf):
        """scores above 0.15 per (frame, class) row"""
        return (conf[..., 1:] > 0.15).sum(1)


SMALL = ((9, 9), (5, 5))      # 318 priors: the smallest head with P >= 200


@pytest.mark.gpu
def test_random_logits_sparse_rows(gpu_lib):
    h = _Head(SMALL, 2, 1)
    for l in h.logits:
        l[..., 41:] -= 8.0   # (the upper half of the classes: rows without a candidate)
    conf, masks, found = h.compare(gpu_lib, torch_too=True)
    n = h.row_counts(conf)
    assert int(n.max()) < K and int((n == 0).sum()) > 0 and int((n > 0).sum()) > 40   # sparse rows, empty ones among them
    assert bool(found.all()) and int((masks > 0).sum()) > 0


@pytest.mark.gpu
def test_more_than_200_candidates_in_a_row(gpu_lib):
    h = _Head(SMALL, 2, 2)
    for l in h.logits:
        l[..., 1] += 10.0
    conf, masks, found = h.compare(gpu_lib, torch_too=True)
    assert int(h.row_counts(conf)[:, 0].min()) > K   # truncation at rank 200 decides
    assert bool(found.all()) and int((masks > 0).sum()) > 0


@pytest.mark.gpu
def test_equal_scores_across_rank_200_and_rank_15(gpu_lib):
    """Level 0's 81 cells repeat four cells' logits: 243 priors share twelve person scores, so the 15th and the 200th place of the person
    row both fall inside a run of equal scores (lowest prior first on either path); the boxes differ with the priors."""
    h = _Head(SMALL, 2, 3)
    for l in h.logits:
        l[..., 1] += 10.0
    h.logits[0][:] = h.logits[0][:, :4].repeat(1, 21, 1, 1)[:, :81]
    conf, masks, found = h.compare(gpu_lib)
    person = conf[0, :, 1]
    top = person.sort(descending=True)[0]
    assert int((person > 0.15).sum()) > K and float(top[K - 1]) == float(top[K]) and float(top[14]) == float(top[15])
    assert bool(found.all()) and int((masks > 0).sum()) > 0


@pytest.mark.gpu
def test_a_frame_with_nothing_above_the_score_threshold(gpu_lib):
    h = _Head(SMALL, 2, 4)
    for l in h.logits:
        l[0, ..., 0] += 40.0    # frame 0: background everywhere
    conf, masks, found = h.compare(gpu_lib, torch_too=True)
    assert float(conf[0, :, 1:].max()) <= 0.15 and int(h.row_counts(conf)[0].sum()) == 0
    assert found.cpu().tolist() == [0, 1] and int(masks[0].sum()) == 0 and int((masks[1] > 0).sum()) > 0


@pytest.mark.gpu
def test_a_list_longer_than_the_sorted_ones(gpu_lib):
    """18 x 18 + 9 x 9 cells (1 215 priors), the person class biased: its rows hold more than kTopkList entries and take the radix select;
    frame 1 repeats cells, so the select has to split runs of equal scores by the prior index."""
    h = _Head(((18, 18), (9, 9)), 2, 5)
    for l in h.logits:
        l[..., 1] += 12.0
    h.logits[0][1] = h.logits[0][1, :6].repeat(54, 1, 1)
    conf, masks, found = h.compare(gpu_lib, torch_too=False)
    n = h.row_counts(conf)
    assert int(n[:, 0].min()) > K_LIST and int(n[:, 1:].max()) < K_LIST
    assert bool(found.all()) and int((masks > 0).sum()) > 0


@pytest.mark.gpu
def test_topk_lists_kernel_against_a_numpy_sort(gpu_lib):
    """amos_mask_topk_lists_device alone: lists with runs of equal scores, counts on both sides of k and of kTopkList (and one long list of ONE
    score, which the select has to split by index alone), in three shuffled orders: the same output, equal to a numpy sort by score
    descending, index ascending; slots past the count hold -1 / 0."""
    rng = np.random.default_rng(7)
    counts = [0, 1, 63, 64, 65, K - 1, K, K + 1, 256, 257, K_LIST - 1, K_LIST, K_LIST + 1, 3000, 1500]
    cap, rows = 3000, len(counts)
    scores = [(rng.integers(8, 48, n) / 50.0).astype(np.float32) for n in counts]
    scores[-1][:] = 0.5
    index = [rng.permutation(5000)[:n].astype(np.uint32) for n in counts]
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for k in (K, 256, 1):
        want_v, want_i = np.full((rows, k), -1.0, np.float32), np.zeros((rows, k), np.int64)
        for r, n in enumerate(counts):
            order = np.lexsort((index[r], -scores[r].astype(np.float64)))[:k]
            want_v[r, :len(order)], want_i[r, :len(order)] = scores[r][order], index[r][order]
        for shuffle in range(3):
            entries = np.full((rows, cap), 0xA5A5A5A5A5A5A5A5, np.uint64)   # (stale bytes past every count)
            for r, n in enumerate(counts):
                perm = rng.permutation(n)
                key = scores[r][perm].view(np.uint32).astype(np.uint64) | np.uint64(0x80000000)   # positive floats: the sign bit set
                entries[r, :n] = (key << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - index[r][perm].astype(np.uint64))
            d_entries = torch.from_numpy(entries.view(np.int64)).cuda()
            d_counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
            v = torch.full((rows, k), float("nan"), device="cuda")
            i = torch.full((rows, k), -7, dtype=torch.int64, device="cuda")
            gpu_lib.mask_topk_lists(st, d_counts.data_ptr(), d_entries.data_ptr(), cap, v.data_ptr(), i.data_ptr(), rows, k)
            torch.cuda.synchronize()
            assert np.array_equal(v.cpu().numpy(), want_v) and np.array_equal(i.cpu().numpy(), want_i), (k, shuffle)
            outs.append(k)
    assert len(outs) == 9
    with pytest.raises(gpu_lib.AmosError):
        gpu_lib.mask_topk_lists(st, d_counts.data_ptr(), d_entries.data_ptr(), cap, v.data_ptr(), i.data_ptr(), rows, 257)


def _spy_head(gpu_lib, monkeypatch):
    """Records the prior offset of every mask_head_candidates call."""
    seen = []
    real = gpu_lib.mask_head_candidates
    monkeypatch.setattr(gpu_lib, "mask_head_candidates", lambda *a: (seen.append(a[-1]), real(*a))[1])
    return seen


@pytest.mark.gpu
def test_engine_pass_with_lists_equals_the_dense_pass(mask, gpu_lib, engine, monkeypatch):
    """The detector's own pass on two golden frames: AMOS_MASK_CANDIDATES on (the default) against off, with side streams and on one stream,
    each pass twice.  Bit-identical masks and `found` throughout."""
    frames = torch.from_numpy(np.stack([mask_cases.frame(c) for c in ("seed0", "ref122_w0")])).cuda()
    seen = _spy_head(gpu_lib, monkeypatch)
    got = {}
    with torch.no_grad():
        x = engine._preprocess_hip(frames)
        for mode, branches in (("1", "auto"), ("0", "auto"), ("1", "0")):
            monkeypatch.setenv("AMOS_MASK_CANDIDATES", mode)
            monkeypatch.setenv("AMOS_MASK_BRANCHES", branches)
            del seen[:]
            masks, found = engine._masks_of(x, 640, 480)
            masks, found = masks.clone(), found.clone()
            again, found2 = engine._masks_of(x, 640, 480)
            torch.cuda.synchronize()
            assert torch.equal(masks, again) and torch.equal(found, found2)
            assert len(seen) == (10 if mode == "1" else 0) and (mode == "0" or min(seen) == 0)   # five levels per pass, or the dense head
            got[(mode, branches)] = (masks, found)
    want = got[("0", "auto")]
    assert bool(want[1].all()) and int((want[0] > 0).sum()) > 0
    for key in (("1", "auto"), ("1", "0")):
        assert torch.equal(got[key][0], want[0]) and torch.equal(got[key][1], want[1]), key


@pytest.mark.gpu
def test_frame_session_graph_with_lists_equals_the_eager_pass(mask, gpu_lib, engine, monkeypatch):
    """The one-frame HIP graph of FrameSession (the counters' memset recorded ahead of the side-stream fork) against the eager one-frame pass
    on a golden frame, replayed on changing frames: bit-identical masks."""
    frames = torch.from_numpy(np.stack([mask_cases.frame(c) for c in ("seed0", "ref122_w0")])).cuda()
    seen = _spy_head(gpu_lib, monkeypatch)
    session = engine.frame_session(480, 640)
    assert len(seen) == 4 * 5   # three warm-up passes and the capture, five levels each
    with torch.no_grad():
        x = engine._preprocess_hip(frames)
        eager = [engine._masks_of(x[k:k + 1], 640, 480)[0][0].clone() for k in range(2)]
    for k in (1, 0, 1):
        session.frame_in.copy_(frames[k].cpu())
        assert session.run() is True
        assert torch.equal(session.mask_out.cuda(), eager[k]) and int((eager[k] > 0).sum()) > 0, k
