"""The hand case of tests/point_choice_cases.py on the GPU: k_motion_accept and k_reloc_accept against the restatement output that
tests/test_point_choice_cpu.py holds to the oracle.  B is accepted on its second feature with that feature's angle, C on the feature of
the new search, D finds nothing; a wrong angle source would clear match[1] or match[2]."""
import numpy as np
import pytest

import motion_model_restatement as mr
import point_choice_cases as cc
import reloc_restatement as rr
import test_gpu_motion_model as motion_gpu  # check
import test_gpu_reloc_search as reloc_gpu   # check

pytestmark = pytest.mark.gpu


def test_motion_model(gpu_lib):
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    kps, desc = cc.frame()
    pts = cc.motion_points(cc.motion_queries(kps, desc))
    cam = mr.camera(eye, zero, eye, zero, 512.0, 512.0, 320.0, 240.0, th=7.0, retry_below=0)
    stats, want = motion_gpu.check(gpu_lib, [(kps, desc, np.full(len(kps), -1, np.float32))], [pts], [cam], mr.HAND_SCALE, mr.HAND_BOUNDS, False)
    m = want[0]["match"]  # check() has held the device's d_match to it
    assert list(m[:3]) == [0, 1, 2] and list(m[20:24]) == [4, 5, 6, 7] and (m >= 0).sum() == 7
    assert (stats["n_matches"][0], stats["n_researched"][0], stats["n_projected"][0]) == (7, 2, 8)


def test_relocalisation(gpu_lib):
    kps, desc, pts = cc.reloc_case()
    pair = dict(frame=0, points=np.concatenate(pts), cam=rr.hand_camera(th=3.0, orb_dist=64, check_orientation=1), found=None,
                match_in=np.full(len(kps), -1, np.int32))
    out, want = reloc_gpu.check(gpu_lib, dict(sf=rr.HAND_SCALE, bounds=rr.HAND_BOUNDS), [(kps, desc)], [pair])
    (query, projected, match, stats), = out
    assert list(match[0, :3]) == [0, 1, 2] and list(match[0, 20:24]) == [4, 5, 6, 7] and (match[0, :len(kps)] >= 0).sum() == 7
    assert (stats["n_matches"][0], stats["n_researched"][0], stats["n_projected"][0], stats["n_occupied"][0]) == (7, 2, 8, 0)
