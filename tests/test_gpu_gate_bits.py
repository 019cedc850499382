"""GPU: the batch gates on bit planes (amos_orb_gate_mode 1: k_bits_pack, k_bits_dilate, k_gate<true>) against the grey planes (mode 0:
k_morph31 twice, k_gate<false>) on the same detection, byte for byte, and against the CPU oracle's gate; tests/test_gate_bits_cpu.py
holds the equivalence itself.  Frame sizes: ten full words per row, a partial last word, and a frame barely larger than the 31 x 31
element (62 x 62 is the extractor's minimum); the masks of tests/gate_bits_restatement.py, in caller buffers with padded rows and frames."""
import ctypes as C

import numpy as np
import pytest

import gate_bits_restatement as gb

pytestmark = pytest.mark.gpu

SIZES = {(480, 640): 8, (150, 200): 3, (62, 70): 1}  # (h, w) -> pyramid levels
GROUPS = [("zero", "full", "one pixel"), ("lines", "holes", "borders"), ("values", "noise", "person"), ("sparse noise",)]


def _frames(h, w, n, seed):
    """blocky frames: corners at every level, up to the borders"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        img = np.kron(rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8), dtype=np.uint8), np.ones((8, 8), np.uint8))[:h, :w]
        out.append(np.clip(img.astype(np.int16) + rng.integers(-12, 12, img.shape), 0, 255).astype(np.uint8))
    return np.stack(out)


def _strided(masks, pad_value=255):
    """the masks in one buffer with an offset, padded rows and padded frames; the padding is non-zero (it must not be read as mask)"""
    n, h, w = masks.shape
    row, off = w + 13, 7
    frame = row * h + 101
    host = np.full(off + n * frame, pad_value, np.uint8)
    for f in range(n):
        host[off + f * frame: off + f * frame + row * h].reshape(h, row)[:, :w] = masks[f]
    return host, off, frame, row


class _Bench:
    def __init__(self, gpu_lib, h, w, n):
        import torch
        self.torch, self.lib, self.h, self.w, self.n, self.levels = torch, gpu_lib, h, w, n, SIZES[(h, w)]
        self.frames = _frames(h, w, n, 100 * h + n)
        self.d_frames = torch.from_numpy(self.frames).cuda()
        self.ext = gpu_lib.OrbExtractor(n_features=600, n_levels=self.levels, max_width=w + 37, max_height=h + 5, max_batch=n + 1)
        torch.cuda.synchronize()

    def detect(self):
        self.ext.detect_batch_device(self.d_frames.data_ptr(), self.h * self.w, self.w, self.w, self.h, self.n)

    def run(self, mode, d_masks, off, frame_stride, row_stride, gate=None):
        """detect -> gate in `mode` -> describe; everything the gate leaves behind, as bytes per frame"""
        before = self.lib.orb_gate_mode(mode)
        try:
            self.detect()
            if gate is None:
                self.ext.gate_batch_device(d_masks.data_ptr() + off, frame_stride, row_stride)
            else:
                gate(d_masks.data_ptr() + off, frame_stride, row_stride)
            removed = [self.ext.batch_removed(f) for f in range(self.n)]
            kept = [[self.ext.level_keypoints(l, f) for l in range(self.levels)] for f in range(self.n)]
            self.ext.describe_batch_device()
            self.ext.sync()
            final = [self.ext.batch_fetch(f) for f in range(self.n)]
        finally:
            self.lib.orb_gate_mode(before)
        return removed, kept, final


def _same_runs(a, b, what):
    for f, (ra, rb) in enumerate(zip(a[0], b[0])):
        assert len(ra) == len(rb), f"{what} frame {f}: {len(ra)} / {len(rb)} keypoints removed"
        assert ra.tobytes() == rb.tobytes(), f"{what} frame {f}: removed lists differ"
    for f, (ka, kb) in enumerate(zip(a[1], b[1])):
        for l, (la, lb) in enumerate(zip(ka, kb)):
            assert la.tobytes() == lb.tobytes(), f"{what} frame {f} level {l}: kept lists differ"
    for f, ((ka, da), (kb, db)) in enumerate(zip(a[2], b[2])):
        assert ka.tobytes() == kb.tobytes() and da.tobytes() == db.tobytes(), f"{what} frame {f}: described result differs"


@pytest.fixture(scope="module")
def benches(gpu_lib):
    cache = {}

    def get(h, w, n):
        if (h, w, n) not in cache:
            cache[(h, w, n)] = _Bench(gpu_lib, h, w, n)
        return cache[(h, w, n)]
    return get


def test_mode_switch_returns_the_previous_value(gpu_lib):
    first = gpu_lib.orb_gate_mode(-1)
    assert first in (0, 1)
    assert gpu_lib.orb_gate_mode(0) == first and gpu_lib.orb_gate_mode(7) == 0 and gpu_lib.orb_gate_mode(1) == 0
    assert gpu_lib.orb_gate_mode(first) == 1


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "+".join(g).replace(" ", "_"))
@pytest.mark.parametrize("size", list(SIZES), ids=lambda s: f"{s[1]}x{s[0]}")
def test_bit_gate_equals_grey_gate_and_oracle(gpu_lib, benches, ob, synth, size, group):
    h, w = size
    n = len(group)  # batches of 3 and of 1
    b = benches(h, w, n)
    all_masks = gb.masks(h, w, synth)
    masks = np.stack([all_masks[name] for name in group])
    host, off, frame_stride, row_stride = _strided(masks)
    d_masks = b.torch.from_numpy(host).cuda()
    b.torch.cuda.synchronize()
    grey = b.run(0, d_masks, off, frame_stride, row_stride)
    bits = b.run(1, d_masks, off, frame_stride, row_stride)
    _same_runs(bits, grey, f"{w}x{h} {group}")
    orc = ob.Oracle(n_features=600, n_levels=b.levels)
    orc.detect(b.frames[0])
    removed = orc.gate(masks[0])
    ko, do = orc.describe()
    assert bits[0][0].tobytes() == removed.tobytes(), "frame 0: removed list differs from the oracle's"
    assert bits[2][0][0].tobytes() == ko.tobytes() and bits[2][0][1].tobytes() == do.tobytes(), "frame 0: result differs from the oracle's"
    if group[0] == "zero":
        assert len(bits[0][0]) == 0  # nothing removed under the empty mask
        assert sum(len(k) for k in bits[1][1]) == 0 and len(bits[2][1][0]) == 0  # everything under the full mask
        assert h < 150 or (len(bits[2][0][0]) > 100 and len(bits[0][1]) > 100)  # (the tiny frame has a handful of corners)


@pytest.mark.parametrize("name", ["borders", "holes", "noise", "values"])
@pytest.mark.parametrize("size", list(SIZES), ids=lambda s: f"{s[1]}x{s[0]}")
def test_bit_gate_at_chosen_pixels(gpu_lib, benches, ob, synth, size, name):
    """The gate's decision pixel by pixel: level 0's list is replaced by keypoints at chosen pixels -- the image's border rows and columns,
    the last word's columns, random ones -- and the removed ones must be those under the oracle's closed mask (closed != 0)."""
    h, w = size
    b = benches(h, w, 1)
    mask = gb.masks(h, w, synth)[name]
    orc = ob.Oracle(n_levels=b.levels)
    orc.detect(b.frames[0])
    orc.gate(mask)
    closed = orc.closed_mask() != 0
    assert np.array_equal(closed, gb.closed_plane(mask))
    b.detect()
    b.ext.sync()
    caps = np.zeros(b.levels, np.int32)
    assert gpu_lib.lib().amos_orb_level_layout(b.ext.h, None, caps.ctypes.data_as(C.c_void_p), None) == 0
    rng = np.random.default_rng(h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    edge = (yy < 2) | (yy >= h - 2) | (xx < 2) | (xx >= w - 17) | ((xx & 63) == 0) | ((xx & 63) == 63)
    pts = np.argwhere(edge)
    pts = pts[rng.permutation(len(pts))[: int(caps[0]) // 2]]
    pts = np.concatenate([pts, np.stack([rng.integers(0, h, int(caps[0]) - len(pts)), rng.integers(0, w, int(caps[0]) - len(pts))], axis=1)])
    kps = np.zeros(len(pts), gpu_lib.KP_DTYPE)
    kps["x"], kps["y"], kps["response"] = pts[:, 1], pts[:, 0], np.arange(len(pts))
    host, off, frame_stride, row_stride = _strided(mask[None])
    d_masks = b.torch.from_numpy(host).cuda()
    b.torch.cuda.synchronize()
    before = gpu_lib.orb_gate_mode(1)
    try:
        b.ext.set_level_keypoints(0, kps)
        b.ext.gate_batch_device(d_masks.data_ptr() + off, frame_stride, row_stride)
        removed = b.ext.batch_removed(0)
        kept = b.ext.level_keypoints(0)
    finally:
        gpu_lib.orb_gate_mode(before)
    want = closed[pts[:, 0], pts[:, 1]]
    level0 = removed[: int(want.sum())]  # the removed list is in level order: level 0's first
    assert level0.tobytes() == kps[want].tobytes(), f"{name} {w}x{h}: removed keypoints are not those under the closed mask"
    assert kept.tobytes() == kps[~want].tobytes(), f"{name} {w}x{h}: kept keypoints are not those outside the closed mask"


def test_labelled_bit_gate_equals_grey_gate(gpu_lib, benches, synth):
    import torch
    n, h, w = 3, 480, 640
    b = benches(h, w, n)
    masks = np.stack([synth.person_mask(3, 4 + k) for k in range(n)])
    masks[1] = 0
    rng = np.random.default_rng(11)
    labels = np.stack([np.kron(rng.integers(1, 49, (15, 20)), np.ones((32, 32))) for _ in range(n)]).astype(np.float64)
    centers = np.zeros((n, 48, 8), np.int32)
    centers[..., 6] = np.arange(1, 49)
    centers[..., 7] = rng.integers(0, 15, (n, 48))
    rm = np.zeros((n, 15), np.int32)
    for f in range(n):
        rm[f, rng.choice(15, 3 + f, replace=False)] = 1
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(l=labels, c=centers, rm=rm).items()}
    host, off, frame_stride, row_stride = _strided(masks)
    d_masks = torch.from_numpy(host).cuda()
    d_status = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def gate(ptr, fs, rs):
        b.ext.gate_labels_batch_device(ptr, fs, rs, d["l"].data_ptr(), h * w, w, d["c"].data_ptr(), 48, 48, d["rm"].data_ptr(), 15, 15, d_status.data_ptr())

    grey = b.run(0, d_masks, off, frame_stride, row_stride, gate)
    assert np.all(d_status.cpu().numpy() == 0)
    d_status.fill_(9)
    bits = b.run(1, d_masks, off, frame_stride, row_stride, gate)
    assert np.all(d_status.cpu().numpy() == 0)
    _same_runs(bits, grey, "label gate")
    plain = b.run(1, d_masks, off, frame_stride, row_stride)
    assert sum(len(r) for r in bits[0]) > sum(len(r) for r in plain[0]) > 0  # the labels remove more than the masks alone


def test_closed_mask_after_a_bit_gate_is_a_state_error(gpu_lib, benches, ob, synth):
    h, w = 480, 640
    b = benches(h, w, 1)
    mask = synth.person_mask(2, 5)
    d_mask = b.torch.from_numpy(mask).cuda()
    b.torch.cuda.synchronize()
    out = np.zeros((h, w), np.uint8)
    b.run(1, d_mask, 0, h * w, w)
    assert b.ext.L.amos_orb_closed_mask(b.ext.h, out.ctypes.data_as(C.c_void_p), w) == -4  # AMOS_ERR_STATE
    assert "bit planes" in gpu_lib.lib().amos_last_error().decode()
    orc = ob.Oracle(n_features=600)
    orc.detect(b.frames[0])
    removed = orc.gate(mask)
    b.run(0, d_mask, 0, h * w, w)  # the grey batch gate leaves frame 0's plane
    assert b.ext.closed_mask().tobytes() == orc.closed_mask().tobytes()
    b.run(1, d_mask, 0, h * w, w)
    before = gpu_lib.orb_gate_mode(1)
    try:
        b.ext.detect(b.frames[0])  # the one-frame gate makes the grey closed mask whatever the mode
        assert b.ext.gate(mask).tobytes() == removed.tobytes()
        assert b.ext.closed_mask().tobytes() == orc.closed_mask().tobytes()
    finally:
        gpu_lib.orb_gate_mode(before)
