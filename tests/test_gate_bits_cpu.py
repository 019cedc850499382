"""CPU: the equivalence the batch gates' bit-plane closing rests on.  k_gate asks closed[iy][ix] != 0 of the grey closing (31 x 31
ellipse, dilate then erode); tests/gate_bits_restatement.py restates the closing of the mask's non-zero set on 64-bit words exactly as
k_bits_pack / k_bits_dilate / bits_closed_at do it.  Both must name the same pixels, for every mask of the GPU test (multi-valued ones
included: a window's maximum is non-zero iff an element is, its minimum iff all are) and at frame sizes with full words, a partial
last word, and a frame barely larger than the element."""
import numpy as np
import pytest

import gate_bits_restatement as gb

SIZES = [(480, 640), (150, 200), (62, 70)]  # (h, w); 62 x 62 is the smallest frame the extractor takes (one level)
NAMES = ["zero", "full", "one pixel", "lines", "holes", "borders", "values", "noise", "sparse noise", "person"]


def test_row_half_widths_are_the_ellipse():
    assert gb.MORPH_DX == gb.ellipse_dx()


def test_pack_layout():
    m = np.zeros((3, 70), np.uint8)
    m[0, 0], m[1, 63], m[2, 64], m[2, 69] = 1, 254, 255, 7
    p = gb.pack(m)
    assert p.shape == (3, 2) and p.dtype == np.uint64
    assert p.tolist() == [[1, 0], [1 << 63, 0], [0, 1 | (1 << 5)]]


@pytest.fixture(scope="module")
def oracles(ob, synth):
    """One detected oracle per frame size (the gate needs a detection; the closed mask does not depend on it)."""
    out = {}
    for h, w in SIZES:
        levels = 8 if (h, w) == (480, 640) else 3 if h >= 150 else 1
        orc = ob.Oracle(n_levels=levels)
        orc.detect(synth.frame(3, 4, h, w))
        out[(h, w)] = orc
    return out


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_bit_closing_names_the_pixels_of_the_grey_closing(oracles, synth, size, name):
    h, w = size
    mask = gb.masks(h, w, synth)[name]
    orc = oracles[size]
    orc.gate(mask)
    want = orc.closed_mask() != 0
    got = gb.closed_plane(mask)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{name} {w}x{h}: {len(bad)} pixels differ, first (y, x) = {bad[0].tolist()}"
    assert (got | (mask == 0)).all()  # a closing removes nothing
    if name == "zero":
        assert not got.any()
    if name == "full":
        assert got.all()


def test_dilated_plane_keeps_its_padding_clear(synth):
    for h, w in SIZES[1:]:
        dil = gb.dilate(gb.pack(gb.masks(h, w, synth)["full"]), w)
        valid = w - 64 * (dil.shape[1] - 1)
        assert int(dil[:, -1].max()) == (1 << valid) - 1
