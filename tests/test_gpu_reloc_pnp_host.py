"""ORB_SLAM2::DevicePnPsolver (amos-slam_amd/host/FrameRelocalizationPnP.h) on stand-in Frame / MapPoint objects, driven through
tests/host_reloc_pnp: constructor, SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) and three iterate(5) calls return the restatement's
Tcw, vbInliers, nInliers and bNoMore."""
import numpy as np
import pytest

import host_reloc_pnp_binding as hp
import reloc_pnp_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["n0", "n9", "n15", "n20", "n65", "n200", "out70", "refine_fails", "duplicates", "duplicates_outliers"])
def test_drop_in_equals_the_restatement_over_three_calls(gpu_lib, name):
    """vpMapPointMatches[i] is the point the case's SearchByBoW row names; a point with the skip bit is a bad MapPoint."""
    pair, seed, want = rc.case(name)
    bad = (pair["points"]["flags"] & 1).astype(np.uint8)
    calls, ms = hp.dropin(gpu_lib, pair["kps"], pair["K"], rc.LEVEL_SIGMA2, pair["points"]["pos"], bad, pair["bow_match"], seed, rc.REFERENCE,
                          rc.N_ITERATIONS, rc.N_CALLS)
    for call, (got, (w, _)) in enumerate(zip(calls, want)):
        print(name, call, "pose", got["has_pose"], "bNoMore", got["no_more"], "nInliers", got["n_inliers"], f"{ms:.3f} ms per iterate")
        assert (got["has_pose"], got["no_more"], got["n_inliers"]) == (w.has_pose, w.no_more, w.n_inliers), (name, call)
        assert got["inliers"].tobytes() == w.inlier.tobytes(), (name, call)
        if w.has_pose:
            assert got["Tcw"][:12].tobytes() == w.Tcw.tobytes() and got["Tcw"][12:].tolist() == [0.0, 0.0, 0.0, 1.0], (name, call)
        else:
            assert not got["Tcw"].any(), (name, call)
