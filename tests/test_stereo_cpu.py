"""Frame::ComputeStereoMatches without a GPU: the sequential restatement (tests/stereo_restatement.py) on the CPU oracle's extraction of a
synthetic rectified pair and on crafted keypoints for the branches that pair does not take, and the new entry points in the library."""
import ctypes

import numpy as np
import pytest

import stereo_restatement as sr

# size, features, levels -> accepted before the median, median-rejected, kept, descriptor-gate rejects, window-end rejects: the counts of
# the prototype restatement this file's was checked against (stream 3, disparities 12 and 31, noise seed 99)
SIZES = {(640, 480, 1000, 8): (694, 186, 508, 296, 13), (322, 241, 500, 6): (342, 93, 249, 144, 16), (160, 120, 300, 4): (110, 29, 81, 47, 1)}
MBF = 40.0


@pytest.mark.parametrize("w,h,nf,nl", list(SIZES))
def test_restatement_on_a_synthetic_pair(ob, w, h, nf, nl):
    left, right = sr.stereo_pair(3, h, w, 12, 31, 99)
    kl, dl, pl, tb = sr.oracle_side(ob, left, nf, 1.2, nl)
    kr, dr, pr, _ = sr.oracle_side(ob, right, nf, 1.2, nl)
    ur, depth, sad, status, st = sr.compute_stereo_matches(kl, dl, kr, dr, pl, pr, tb["scale"], tb["inv_scale"], h, MBF, MBF / min(w, 525))
    kept = ur >= 0
    print(w, h, len(kl), len(kr), st, int(kept.sum()))
    assert status == 0
    assert np.array_equal(kept, depth > 0) and np.array_equal(sad >= 0, (sad >= 0) | kept)
    disparity = kl["x"][kept] - ur[kept]
    half = np.where(kl["y"][kept] < h // 2, 12.0, 31.0)
    near = (np.abs(disparity - 12) <= 2) | (np.abs(disparity - 31) <= 2)
    assert (~near).sum() <= 0.03 * kept.sum(), (int((~near).sum()), int(kept.sum()))
    assert (np.abs(disparity - half) <= 2).mean() > 0.9   # and the disparity is the one of the keypoint's half of the image
    assert np.array_equal(depth[kept], (np.float32(MBF) / (kl["x"][kept] - ur[kept])).astype(np.float32))
    assert kept.sum() >= 0.4 * len(kl)
    assert (st["accepted"], st["median_rejected"], int(kept.sum()), st["desc_gate"], st["window_end"]) == SIZES[(w, h, nf, nl)]
    if w == 640:
        assert st["desc_gate"] > 0 and st["window_end"] > 0 and st["median_rejected"] > 0
    assert st["border"] == st["delta"] == st["disparity"] == st["tiny_disparity"] == 0  # hence the hand cases below


@pytest.fixture(scope="module")
def hand(ob):
    cases = sr.hand_cases(ob)
    return {name: (c, sr.run_hand_case(ob, c)) for name, c in cases.items()}


def test_hand_border(hand):
    _, (ur, depth, sad, status, st) = hand["border"]
    assert st["border"] == 2 and (ur == -1).all() and (depth == -1).all() and (sad == -1).all() and status == 0


def test_hand_identical_images(hand):
    """disparity = -deltaR: negative ones leave at :1515; the others are accepted with SAD 0, so the median is 0 and thDist rejects them all"""
    c, (ur, depth, sad, status, st) = hand["identical"]
    assert st["disparity"] > 0 and st["accepted"] > 0 and st["disparity"] + st["accepted"] == len(c["kps_l"])
    assert (sad[sad >= 0] == 0).all() and st["median_rejected"] == st["accepted"] and (ur == -1).all()


def test_hand_symmetric_zero_disparity(hand):
    c, (ur, depth, sad, status, st) = hand["symmetric"]
    assert st["tiny_disparity"] == 1 and st["accepted"] == 4 and st["median_rejected"] == 0
    uL = c["kps_l"]["x"][0]
    assert sad[0] == 0
    assert ur[0].tobytes() == np.float32(float(uL) - 0.01).tobytes()
    assert depth[0].tobytes() == (np.float32(sr.HAND_MBF) / np.float32(0.01)).astype(np.float32).tobytes()
    assert (np.abs(c["kps_l"]["x"][1:] - ur[1:] - 7) < 1).all()


def test_hand_flat_patch_and_empty_right(hand):
    _, (ur, depth, sad, status, st) = hand["flat"]
    assert st["window_end"] == 1 and ur[0] == -1 and depth[0] == -1 and sad[0] == -1
    c, (ur, depth, sad, status, st) = hand["empty_right"]
    assert len(ur) == len(c["kps_l"]) > 0 and (ur == -1).all() and (depth == -1).all() and (sad == -1).all() and st["accepted"] == 0


def test_hand_out_of_range(hand):
    _, (ur, depth, sad, status, st) = hand["out_of_range"]
    assert status == 1 and list(ur >= 0) == [False, False, False, True, False]


def test_parabola_denominator_is_positive():
    """The issue's NaN case (d1 == d3 and d1 + d3 == 2 d2) and the infinite deltaR cannot be built: the best shift is the FIRST strict
    minimum, so for an interior best d1 > d2 and d3 >= d2, the denominator 2 ((d1 - d2) + (d3 - d2)) is positive and deltaR lies in
    (-0.5, 0.5].  The comparisons of :1499 and :1515 are restated all the same.  Checked here over every SAD triple order and at random."""
    rng = np.random.default_rng(1)
    for _ in range(2000):
        d = rng.integers(0, 4, 11)  # small range: many ties
        best, inc = 2 ** 31 - 1, 0
        for i, v in enumerate(d):
            if v < best:
                best, inc = v, i
        if inc in (0, 10):
            continue
        d1, d2, d3 = (np.float32(d[inc - 1]), np.float32(d[inc]), np.float32(d[inc + 1]))
        den = np.float32(2) * (d1 + d3 - np.float32(2) * d2)
        assert den > 0 and -0.5 < (d1 - d3) / den <= 0.5


def test_library_exports_the_stereo_entry_points(pkg):
    names = ("amos_frame_stereo_match_batch_device", "amos_frame_stereo_match_arrays_device")
    lib = ctypes.CDLL(pkg.LIB_PATH)
    for name in names:
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    assert hasattr(pkg.OrbExtractor, "stereo_match_batch_device") and hasattr(pkg.OrbExtractor, "stereo_match_arrays_device")
