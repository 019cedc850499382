"""CPU side of tests/test_gpu_scene_flow_sweep.py: what must hold for the ORACLE ALONE so that the GPU sweep is worth its name (its
inputs fall where the module says they fall), and the calls of the scene-flow front that are refused before the device is opened."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import flow_oracle as fo  # noqa: E402

import test_gpu_scene_flow_sweep as sweep  # noqa: E402


def test_flow_check_scene_facts(synth):
    """the 67 x 43 scene: the hand-placed pairs fall either side of the four 5-px limits as described there, the extreme-SAD pair (2295,
    the most nine 8-bit pixels can differ by) is kept, the rest is mixed"""
    last, cur, pre, nxt, state = sweep.flow_scene(synth)
    want = fo.flow_check(last, cur, pre, nxt, state)
    assert want[:17].tolist() == [1] + [0, 1, 1, 0] * 4
    assert int(np.abs(last[20:23, 30:33].astype(int) - cur[20:23, 30:33].astype(int)).sum()) == sweep.SAD_MAX < 2520 and want[17] == 1
    assert 0 < want[18:].sum() < len(want[18:]) and ((want == 0) & (state == 1)).sum() > 8 and (state == 0).sum() > 8


def test_lk_grid_reaches_top_levels_0_to_4(ob, synth):
    """buildOpticalFlowPyramid's level count varies over the window x max_level grid"""
    tops = set()
    for w, h in sweep.LK_FRAMES:
        a, b = sweep.lk_pair(synth, w, h)
        for win in sweep.LK_WINDOWS:
            for ml in sweep.LK_LEVELS:
                tops.add(ob.lk_track(a, b, sweep.lk_points(w, h, 4), win=win, max_level=ml)[3])
    assert tops == {0, 1, 2, 3, 4}


def test_chain_image_oracle_facts(ob):
    """the dependency chain: 80 corners at distance 1, every second blob (10) at distance 7"""
    img = sweep.chain_image()
    assert len(ob.good_features_to_track(img, max_corners=0, quality=1e-4, min_distance=1.0)) == 80
    chain = ob.good_features_to_track(img, max_corners=0, quality=1e-4, min_distance=7.0)
    assert chain[:, 0].tolist() == [6.0 + 12 * i for i in range(10)]


def test_creation_refuses_bad_windows_and_small_frames(pkg):
    """amos_lk_create / amos_corners_create validate before they open the device: return codes only, with or without a GPU"""
    for w, h, win in ((640, 480, 2), (640, 480, 23), (22, 480, 22), (640, 22, 22), (15, 15, 15), (3, 100, 3)):
        with pytest.raises(pkg.AmosError, match=r"rc=-1"):
            pkg.LkTracker(w, h, win_size=win)
    for ml in (-1, 8):
        with pytest.raises(pkg.AmosError, match=r"rc=-1"):
            pkg.LkTracker(640, 480, max_level=ml)
    with pytest.raises(pkg.AmosError, match=r"rc=-1"):
        pkg.CornerDetector(max_width=7, max_height=480)
