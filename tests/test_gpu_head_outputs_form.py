"""k_head_outputs<true> with a thread per (anchor, class) column (amos_mask_head_form_mode 1) against its element loops (mode 0), through
amos_mask_head_candidates_device: the same loc (and coef) bytes and, after sorting, the same entries in every (frame, class) list.  Cells
below, at and above the 16 a work-group stages (one group, a full one, a second one with one cell, with nine), the 256-channel layer without
coefficients and the 384-channel one with them, a threshold nothing passes, one everything passes, the display threshold, and a NaN."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ANCHORS, C1, DIM, BATCH = 3, 81, 32, 2
OFFSET, EXTRA = 5, 4   # the level's priors start at prior 5 of the concatenated outputs, four more follow them


def _raw(cells, with_coef, seed, nan):
    g = torch.Generator().manual_seed(seed)
    cpad = 384 if with_coef else 256
    used = ANCHORS * (4 + C1 + (DIM if with_coef else 0))
    raw = torch.zeros(BATCH, cells, cpad)
    raw[..., :used] = torch.randn(BATCH, cells, used, generator=g) * 2
    if nan:
        raw[1, cells // 2, ANCHORS * 4 + C1 + 7] = float("nan")   # a class value of the middle cell's second anchor, frame 1
    bias = torch.randn(cpad, generator=g) * 0.1
    bias[used:] = 0
    return raw.cuda(), bias.cuda()


def _run(lib, raw, bias, with_coef, threshold, mode):
    cells, cpad = raw.shape[1], raw.shape[2]
    P = OFFSET + cells * ANCHORS + EXTRA
    C = C1 - 1
    st = torch.cuda.current_stream().cuda_stream
    loc = torch.full((BATCH, P, 4), -3.0, device="cuda")
    coef = torch.full((BATCH, P, DIM), -3.0, device="cuda") if with_coef else None
    cand = torch.full((lib.mask_candidates_bytes(BATCH, P, C1),), 0xA5, dtype=torch.uint8, device="cuda")
    before = lib.mask_head_form_mode(mode)
    try:
        lib.mask_candidates_reset(st, cand.data_ptr(), BATCH, C1)
        lib.mask_head_candidates(st, raw.data_ptr(), bias.data_ptr(), loc.data_ptr(), coef.data_ptr() if with_coef else None, cand.data_ptr(), threshold, BATCH,
                                 cells, cpad, ANCHORS, C1, DIM, P, OFFSET)
        torch.cuda.synchronize()
    finally:
        lib.mask_head_form_mode(before)
    buf = cand.cpu().numpy()
    counts = buf[:BATCH * C * 4].view(np.int32).copy()
    head = (BATCH * C * 4 + 255) // 256 * 256
    entries = buf[head:].view(np.uint64).reshape(BATCH * C, P)
    lists = [np.sort(entries[r, :counts[r]]) for r in range(BATCH * C)]
    return loc.cpu().numpy(), None if coef is None else coef.cpu().numpy(), counts, lists


CASES = [(cells, with_coef) for cells in (1, 15, 16, 17, 25) for with_coef in (False, True)]


@pytest.mark.parametrize("cells,with_coef", CASES, ids=[f"{c}_cells_cpad_{384 if w else 256}" for c, w in CASES])
def test_column_form_equals_the_element_loops(gpu_lib, cells, with_coef):
    for threshold, nan, expect in ((1.0, False, "nothing"), (0.0, False, "everything"), (0.15, False, "some"), (0.15, True, "some")):
        raw, bias = _raw(cells, with_coef, 100 * cells + int(with_coef), nan)
        old = _run(gpu_lib, raw, bias, with_coef, threshold, 0)
        new = _run(gpu_lib, raw, bias, with_coef, threshold, 1)
        case = (cells, with_coef, threshold, nan)
        assert new[0].tobytes() == old[0].tobytes(), case
        if with_coef:
            assert new[1].tobytes() == old[1].tobytes(), case
        assert np.array_equal(new[2], old[2]), case
        for r, (a, b) in enumerate(zip(new[3], old[3])):
            assert np.array_equal(a, b), (case, r)
        # what the case is there for: the priors outside the level untouched, loc = raw + bias, and the lists empty / full / in between
        lo = old[0]
        assert bool((lo[:, :OFFSET] == -3.0).all()) and bool((lo[:, OFFSET + cells * ANCHORS:] == -3.0).all())
        want_loc = (raw[..., :ANCHORS * 4] + bias[:ANCHORS * 4]).reshape(BATCH, cells * ANCHORS, 4).cpu().numpy()
        assert lo[:, OFFSET:OFFSET + cells * ANCHORS].tobytes() == want_loc.tobytes(), case
        total, every = int(old[2].sum()), BATCH * cells * ANCHORS * (C1 - 1)
        if expect == "nothing":
            assert total == 0
        elif expect == "everything":
            assert total == every   # (a softmax quotient of these values is never zero: |raw + bias| stays below 12)
        else:
            assert 0 < total < every
            if nan:   # the prior with the NaN has a NaN sum: none of its classes passes; every other prior as without the NaN
                clean = _run(gpu_lib, *_raw(cells, with_coef, 100 * cells + int(with_coef), False), with_coef, threshold, 1)
                prior = OFFSET + (cells // 2) * ANCHORS + 1
                key = np.uint64(0xFFFFFFFF - prior)
                for r in range(BATCH * (C1 - 1)):
                    kept = clean[3][r][(clean[3][r] & np.uint64(0xFFFFFFFF)) != key] if r >= C1 - 1 else clean[3][r]
                    assert np.array_equal(old[3][r], kept), (case, r)


def test_mode_switch_returns_the_previous_value(gpu_lib):
    first = gpu_lib.mask_head_form_mode(-1)
    assert first in (0, 1)
    try:
        assert gpu_lib.mask_head_form_mode(0) == first and gpu_lib.mask_head_form_mode(5) == 0 and gpu_lib.mask_head_form_mode(1) == 0
        assert gpu_lib.mask_head_form_mode(-1) == 1
    finally:
        gpu_lib.mask_head_form_mode(first)
