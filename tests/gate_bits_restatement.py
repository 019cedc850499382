"""numpy restatement of the batch gates' closing on bit planes (csrc/orb_kernels.h: k_bits_pack, k_bits_dilate, bits_closed_at), with the
kernels' words, shifts and border rules, and the masks the two gate tests share.

A plane is [rows][ceil(W / 64)] uint64, bit b of word k = pixel 64 k + b, bits at x >= W are 0.  The dilation treats everything outside
the image as 0; the erosion treats rows outside it and columns outside it as set."""
import numpy as np

MORPH_DX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 7, 5, 0)  # half-width of element row |dy| (kMorphDx)
_U = np.uint64
_ALL = _U(0xFFFFFFFFFFFFFFFF)


def ellipse_dx():
    """getStructuringElement(MORPH_ELLIPSE, 31 x 31)'s row half-widths, computed as OpenCV does."""
    r = 15
    return tuple(int(np.rint(r * np.sqrt((r * r - dy * dy) / float(r * r)))) for dy in range(16))


def pack(mask):
    """k_bits_pack: mask != 0, one bit per pixel."""
    h, w = mask.shape
    words = (w + 63) // 64
    bits = np.zeros((h, words * 64), np.uint64)
    bits[:, :w] = mask != 0
    weights = _U(1) << np.arange(64, dtype=np.uint64)
    return (bits.reshape(h, words, 64) * weights).sum(axis=2, dtype=np.uint64)


def dilate(packed, w):
    """k_bits_dilate: the rows by |dy| = 0 .. 15 into one 128-bit accumulator per word (lo, hi), widened between two half-widths."""
    h, words = packed.shape
    zero_col = np.zeros((h, 1), np.uint64)
    left = np.concatenate([zero_col, packed[:, :-1]], axis=1)    # word k - 1, 0 before the first
    right = np.concatenate([packed[:, 1:], zero_col], axis=1)    # word k + 1, 0 after the last
    row_lo = (left >> _U(32)) | (packed << _U(32))
    row_hi = (packed >> _U(32)) | (right << _U(32))

    def shifted_rows(a, dy):  # a[y + dy], 0 outside the image
        out = np.zeros_like(a)
        if dy >= 0:
            out[:h - dy] = a[dy:] if dy < h else 0
        else:
            out[-dy:] = a[:h + dy] if -dy < h else 0
        return out

    lo, hi = np.zeros_like(packed), np.zeros_like(packed)
    for a in range(16):
        if a > 0 and MORPH_DX[a] != MORPH_DX[a - 1]:
            d, r = MORPH_DX[a - 1] - MORPH_DX[a], 0
            while r < d:  # v | v << s | v >> s widens a set already widened by r without gaps while s <= 2 r + 1
                s = _U(min(d - r, 2 * r + 1))
                e = _U(64) - s
                ll, lh, rl, rh = lo << s, (hi << s) | (lo >> e), (lo >> s) | (hi << e), hi >> s
                lo, hi = lo | ll | rl, hi | lh | rh
                r += int(s)
        for dy in ((0,) if a == 0 else (-a, a)):
            if abs(dy) < h:
                lo |= shifted_rows(row_lo, dy)
                hi |= shifted_rows(row_hi, dy)
    out = (lo >> _U(32)) | (hi << _U(32))
    valid = w - 64 * (words - 1)
    if valid < 64:
        out[:, -1] &= (_U(1) << _U(valid)) - _U(1)
    return out


def closed_at(dil, w, ix, iy):
    """bits_closed_at for arrays of pixel coordinates: the erosion of the dilated plane at (iy, ix), the window clipped to the image."""
    h = dil.shape[0]
    ix, iy = np.asarray(ix, np.int64), np.asarray(iy, np.int64)
    ok_all = np.ones(ix.shape, bool)
    for dy in range(-15, 16):
        r = MORPH_DX[abs(dy)]
        yy = iy + dy
        inside = (yy >= 0) & (yy < h)
        row = np.where(inside, yy, iy)
        x0, x1 = np.maximum(ix - r, 0), np.minimum(ix + r, w - 1)
        k0, k1 = x0 >> 6, x1 >> 6
        m0 = _ALL << (x0 & 63).astype(np.uint64)
        m1 = _ALL >> (63 - (x1 & 63)).astype(np.uint64)
        same = k0 == k1
        a, b = np.where(same, m0 & m1, m0), np.where(same, m0 & m1, m1)
        ok = ((dil[row, k0] & a) == a) & ((dil[row, k1] & b) == b)
        ok_all &= ok | ~inside
    return ok_all


def closed_plane(mask):
    """closed != 0 of the whole mask, as k_gate<true> sees it pixel by pixel."""
    h, w = mask.shape
    yy, xx = np.mgrid[0:h, 0:w]
    return closed_at(dilate(pack(mask), w), w, xx.ravel(), yy.ravel()).reshape(h, w)


def masks(h, w, synth):
    """The masks of the gate tests at one frame size, name -> uint8 [h][w]."""
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"zero": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8)}
    m = np.zeros((h, w), np.uint8)
    m[h // 2, w // 3] = 255
    out["one pixel"] = m
    m = np.zeros((h, w), np.uint8)
    m[h // 4: 3 * h // 4, w // 2] = 255
    m[h // 3, w // 8: 7 * w // 8] = 255
    out["lines"] = m
    m = np.zeros((h, w), np.uint8)  # a blob with a hole the element fills (radius 6) and one with a hole it does not (radius 22)
    cy, cx, rb = h // 2, w // 2, min(h, w) // 2 - 2
    m[(yy - cy) ** 2 + (xx - cx) ** 2 <= rb * rb] = 255
    m[(yy - cy + rb // 2) ** 2 + (xx - cx) ** 2 <= 36] = 0
    if rb > 30:
        m[(yy - cy - rb // 4) ** 2 + (xx - cx) ** 2 <= 22 * 22] = 0
    out["holes"] = m
    m = np.zeros((h, w), np.uint8)  # blobs on the four borders and in a corner, gaps narrower and wider than the element between them
    m[:9, w // 3: w // 3 + 20] = 255
    m[h - 7:, w // 2: w // 2 + 25] = 255
    m[h // 3: h // 3 + 18, :6] = 255
    m[h // 2: h // 2 + 14, w - 5:] = 255
    m[h - 12:, w - 12:] = 255
    m[:4, :4] = 255
    out["borders"] = m
    m = np.zeros((h, w), np.uint8)  # real masks are 255 * n mod 256: several grey levels, 1 among them
    m[(yy - h // 3) ** 2 + (xx - w // 3) ** 2 <= (min(h, w) // 4) ** 2] = 255
    m[(yy - h // 2) ** 2 + (xx - w // 2) ** 2 <= (min(h, w) // 5) ** 2] = 254
    m[2 * h // 3: 2 * h // 3 + 9, w // 5: 4 * w // 5: 3] = 1
    out["values"] = m
    out["noise"] = ((rng.random((h, w)) < 0.5) * rng.choice(np.array([1, 254, 255], np.uint8), (h, w))).astype(np.uint8)
    out["sparse noise"] = ((rng.random((h, w)) < 0.004) * 255).astype(np.uint8)
    out["person"] = synth.person_mask(3, 4, h, w)
    return out
