"""ORB_SLAM2::SearchBySim3 (amos-slam_amd/host/KeyFrameSim3Search.h) on stand-in KeyFrame / MapPoint objects against the restatement
(tests/sim3_search_restatement.py): vpMatches12 on return pointer for pointer, and the return value.  A vpMatches12 entry is a MapPoint
pointer, so the rows here name keyframe-2 features that carry a point; an entry whose point is in neither keyframe (GetIndexInKeyFrame
returns -1) takes the AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE path."""
import numpy as np
import pytest

import host_sim3_search_binding as hsb
import sim3_search_restatement as ss

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["truth", "same", "double", "wide", "empty_1", "empty_2"])
def test_dropin_equals_the_restatement(gpu_lib, name):
    sc, _ = ss.shared()
    p = sc["names"].index(name)
    a, b = int(sc["slots1"][p]), int(sc["slots2"][p])
    kf1, kf2 = ss.keyframe(sc, a), ss.keyframe(sc, b)
    n1, n2 = len(kf1["kps"]), len(kf2["kps"])
    pr = sc["pairs"][p]
    # the row as pointers can say it: a feature of keyframe 2 without a point object cannot be pointed at
    row = sc["rows"][p][:n1].copy()
    has_object = (kf2["points"]["flags"] & (ss.lr.SKIP | ss.BAD)) != ss.lr.SKIP
    for i in range(n1):
        if row[i] >= n2 or (row[i] >= 0 and not has_object[row[i]]):
            row[i] = ss.MATCHED_ELSEWHERE
    want = ss.search(kf1, kf2, sc["cameras"][a], sc["cameras"][b], pr["R12"], pr["t12"], pr["s12"], pr["th"], row, sc["sf"], sc["bounds"])
    s1, keep1 = hsb.standin(kf1, sc["cameras"][a], sc["sf"], sc["bounds"])
    s2, keep2 = (s1, keep1) if a == b else hsb.standin(kf2, sc["cameras"][b], sc["sf"], sc["bounds"])
    found, out, _ = hsb.dropin(s1, s2, row, pr["R12"], pr["t12"], pr["s12"], pr["th"])
    print(name, "found", found, "of", want["stats"])
    assert found == want["stats"]["n_found"]
    assert np.array_equal(out, want["match_out"])
    if n1 and n2:
        elsewhere = row == ss.MATCHED_ELSEWHERE
        assert elsewhere.any() and (out[elsewhere] == ss.MATCHED_ELSEWHERE).all() and (want["reason"][0][elsewhere] <= ss.REASONS["matched"]).all()
        assert found > 0 and ((row >= 0) & (out == row)).any()
