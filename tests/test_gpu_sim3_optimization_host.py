"""The host form amos_match_sim3_optimize and the C++ drop-in ORB_SLAM2::OptimizeSim3 (amos-slam_amd/host/KeyFrameSim3Optimize.h) on stand-in
KeyFrame / MapPoint / Sim3 objects, on the GPU, against the restatement: the returned value, vpMatches1 and g2oS12."""
import numpy as np
import pytest

import pose_optimization_restatement as pr
import sim3_optimization_cases as sc
import sim3_optimization_restatement as so

pytestmark = pytest.mark.gpu

NAMES = ("n20_fix0_out25", "n64_fix1_out0", "n9_fix0_out0", "n300_fix0_out25", "n11_fix1_out25")


def test_host_form_equals_the_restatement(gpu_lib):
    grid, want = sc.shared()
    mt = gpu_lib.OrbMatcher()
    for name in NAMES:
        p = [n for n, _ in grid].index(name)
        s, (res, row) = grid[p][1], want[p]
        got, out = mt.sim3_optimize(s["kps1"], s["pts1"], s["kps2"], s["pts2"], [s["cam1"], s["cam2"]], s["row"], sc.INV_SIGMA2, s["pair"])
        assert np.array_equal(out, row) and got.tobytes() == res.tobytes(), name
    s = grid[0][1]
    off = s["pair"].copy()
    off["enabled"] = 0
    got, out = mt.sim3_optimize(s["kps1"], s["pts1"], s["kps2"], s["pts2"], [s["cam1"], s["cam2"]], s["row"], sc.INV_SIGMA2, off)
    assert got["skipped"] == 1 and got["n_inliers"] == 0 and np.array_equal(out, s["row"])
    empty = sc.scene(0, 0, extra=False)
    got, out = mt.sim3_optimize(empty["kps1"], empty["pts1"], empty["kps2"], empty["pts2"], [empty["cam1"], empty["cam2"]], empty["row"], sc.INV_SIGMA2,
                                empty["pair"])
    assert got.tobytes() == sc.expected(empty)[0].tobytes() and got["rounds"] == 0 and len(out) == 0
    mt.close()


def test_dropin_equals_the_restatement(gpu_lib):
    import host_sim3_optimize_binding as hb
    grid, _ = sc.shared()
    for name in NAMES:
        s = dict(grid[[n for n, _ in grid].index(name)][1])
        # the drop-in hands the device toRotationMatrix(Quaterniond(R12)) rounded to float
        q = pr.quat_from_R([float(v) for v in s["pair"]["R12"]])
        pair = s["pair"].copy()
        pair["R12"] = np.array(pr.quat_to_R(q), np.float64).astype(np.float32)
        res, row = sc.expected(dict(s, pair=pair))
        got = hb.optimize("dropin", s, sc.INV_SIGMA2)
        assert got["ret"] == res["n_inliers"], name
        assert np.array_equal(got["row"], (row != -1).astype(np.int32)), name
        if res["rounds"] == 2:
            assert got["sim3"].tobytes() == np.concatenate([res["q"], res["t"], [res["s"]]]).tobytes(), name
        else:  # 0 ahead of the second optimisation: g2oS12 is as it was
            assert got["sim3"].tobytes() == np.array(q + [float(v) for v in s["pair"]["t12"]] + [float(s["pair"]["s12"])]).tobytes(), name
