"""The greedy choice of the motion-model and the relocalisation search without a GPU, on the hand case of tests/point_choice_cases.py: the
restatements against the CPU oracle and against values worked out here.  tests/test_gpu_point_choice.py holds the device to the same
restatement output.

A (distance 0) takes feature 0.  B (2, 12, 22) finds feature 0 taken and takes feature 1.  C (3, 13, 23) finds both taken, searches
again and gets feature 2.  D (4, 14, 24) finds both taken and nothing free: two points searched again, seven matches.  The bins are 3
(A, B, a filler), 7 (C, a filler) and 9 (two fillers), all three stand.  B's bin comes from feature 1's angle (132 - 96 = 36): from
feature 0's it would be bin 11, a fourth bin of one entry, and match[1] would be cleared; C's from feature 2's (264 - 180 = 84): from
feature 0's or 1's it would be bin 22 or 14 and lose against bin 7 of the same size, the earlier bin."""
import numpy as np

import motion_model_restatement as mr
import point_choice_cases as cc
import reloc_restatement as rr
import test_motion_model_cpu as motion_cpu  # both, TH
import test_reloc_search_cpu as reloc_cpu   # run, oracle_search


def test_the_bins_of_the_case():
    assert [mr.rotation_bin(a, b) for a, b in ((36.0, 0.0), (132.0, 96.0), (264.0, 180.0), (84.0, 0.0), (108.0, 0.0))] == [3, 3, 7, 7, 9]
    assert [mr.rotation_bin(a, b) for a, b in ((132.0, 0.0), (264.0, 0.0), (264.0, 96.0))] == [11, 22, 14]
    for wrong in ([3, 11, 7, 3, 7, 9, 9], [3, 3, 22, 3, 7, 9, 9], [3, 3, 14, 3, 7, 9, 9]):  # a wrong angle source for B, for C
        assert mr.three_maxima(np.bincount(wrong, minlength=30)) in ((3, 7, 9), (3, 9, 7))


def test_motion_model_best_taken_takes_the_second_and_both_taken_search_again(ob):
    kps, desc = cc.frame()
    q = cc.motion_queries(kps, desc)
    r = motion_cpu.both(kps, desc, q)  # the oracle, equal to the Python restatement
    assert r["n_matches"] == 7 and list(r["match"][:3]) == [0, 1, 2] and list(r["match"][20:24]) == [4, 5, 6, 7]
    assert (r["match"] >= 0).sum() == 7 and 3 not in r["match"]
    n, m, researched = mr.search_python(kps, desc, None, q, mr.HAND_SCALE, 40.0, motion_cpu.TH, 0, 0, 1, mr.HAND_BOUNDS)
    assert (n, researched) == (7, 2) and np.array_equal(m, r["match"])


def test_relocalisation_best_taken_takes_the_second_and_both_taken_search_again():
    kps, desc, pts = cc.reloc_case()
    r = reloc_cpu.run(kps, desc, pts, check_orientation=1)
    assert list(r["match"][:3]) == [0, 1, 2] and list(r["match"][20:24]) == [4, 5, 6, 7] and (r["match"] >= 0).sum() == 7
    assert (r["n_matches"], r["n_researched"], r["n_projected"], r["n_occupied"]) == (7, 2, 8, 0)
    assert list(r["query"]["level"][:4]) == [3, 3, 3, 3]
    none = np.full(len(kps), -1, np.int32)
    n, m, q, pidx = reloc_cpu.oracle_search(kps, desc, np.concatenate(pts), rr.hand_camera(th=3.0, orb_dist=64, check_orientation=1),
                                            np.zeros(len(pts), np.uint8), none, rr.HAND_SCALE, rr.HAND_BOUNDS)
    assert n == 7 and np.array_equal(m, r["match"]) and list(pidx) == list(range(8))
