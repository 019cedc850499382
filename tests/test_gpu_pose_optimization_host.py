"""The one-frame host entry amos_match_pose_optimization and the C++ drop-in ORB_SLAM2::PoseOptimization (on the stand-in Frame of
tests/host_pose) against the Python restatement: the same pose, flags and return value, bit for bit."""
import numpy as np
import pytest

import pose_optimization_cases as pc

pytestmark = pytest.mark.gpu

NAMES = ("2_mixed_0", "3_mono_0", "9_mixed_25", "10_stereo_25", "65_mixed_25", "257_mono_25", "1000_mixed_25", "exact_optimum", "zero_depth_stereo",
         "behind", "bad_octave")
FLOAT_FIELDS = ("Rt", "Tcw", "Ow", "lambda", "chi2")
INT_FIELDS = ("n_edges", "n_inliers", "n_inliers_with_obs", "rounds", "status", "iterations", "trials")


@pytest.fixture(scope="module")
def cases():
    allc = pc.all_cases()
    return {k: allc[k] for k in NAMES}


@pytest.mark.parametrize("clear", [0, 1])
def test_host_form_equals_the_restatement(gpu_lib, cases, clear):
    mt = gpu_lib.OrbMatcher()
    for name, c in cases.items():
        n = len(c["kps"])
        entry = np.full(n, 7, np.uint8)
        res, outlier, match = mt.pose_optimization(c["kps"], c["match"], c["pos"], c["camera"], c["inv_sigma2"], outlier=entry, has_obs=c["has_obs"],
                                                   clear_outliers=clear, u_right=c["u_right"])
        w_res, w_outlier, w_match = pc.restate(c, clear, 7)
        for field in FLOAT_FIELDS:
            assert pc.same_bits(res[field], w_res[field]), (name, field)
        for field in INT_FIELDS:
            assert np.array_equal(res[field], w_res[field]), (name, field)
        assert np.array_equal(outlier, w_outlier) and np.array_equal(match, w_match), name
    empty = cases["9_mixed_25"]
    res, outlier, match = mt.pose_optimization(empty["kps"][:0], empty["match"][:0], empty["pos"][:0], empty["camera"], empty["inv_sigma2"])
    assert res["n_edges"] == 0 and res["n_inliers"] == 0 and len(outlier) == len(match) == 0
    assert pc.same_bits(res["Tcw"].reshape(3, 4)[:, :3].reshape(9), empty["camera"]["Rcw"])
    mt.close()


def test_the_drop_in_on_the_stand_in_frame(gpu_lib, cases):
    import host_pose_binding as hp
    for name, c in cases.items():
        n = len(c["kps"])
        entry = (np.arange(n) % 3 == 0).astype(np.uint8)  # mvbOutlier on entry
        got = hp.pose_optimization("dropin", c, outlier=entry)
        w_res, w_outlier, _ = pc.pose_optimization_with_entry(c, entry)
        assert got["ret"] == w_res["n_inliers"], name
        if w_res["n_edges"] < 3:  # Optimizer.cc:506: flags of matched features reset, no SetPose
            want = np.where((c["match"] >= 0) & (np.arange(n) < c["count"]), 0, entry)
            assert got["set_pose"] == 0 and np.array_equal(got["outlier"], want), name
            continue
        assert got["set_pose"] == 1 and pc.same_bits(got["Tcw"], w_res["Tcw"]), name
        assert np.array_equal(got["outlier"], w_outlier), name
        core = hp.pose_optimization("core", c, outlier=entry)  # the same arithmetic compiled for the host
        assert core["ret"] == got["ret"] and pc.same_bits(core["Tcw"], got["Tcw"]) and np.array_equal(core["outlier"], got["outlier"]), name
