"""ORB_SLAM2::SearchLocalPoints (amos-slam_amd/host/FrameLocalPoints.h) on stand-in Frame / MapPoint objects through tests/host_local/:
equal to the chain the host classes had before it -- isInFrustum on the host, point by point, then ORBmatcherFor::SearchByProjection --
on the same objects.  ref_standins.h has no isInFrustum, so the harness writes it (tests/host_local/local_capi.cc, in the reference's
order); what makes the chain independent of the device code is the stand-ins' logarithm-based PredictScale, the host's own arithmetic and
ORBmatcherFor::SearchByProjection (host enumeration, host greedy loop)."""
import numpy as np
import pytest

import local_points_restatement as lr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stereo,th,nn_ratio", [(True, 1.0, 0.8), (False, 3.0, 0.8), (True, 5.0, 0.6)])
def test_dropin_equals_the_host_chain(gpu_lib, ob, synth, stereo, th, nn_ratio):
    import host_local_binding as hl
    nl = 8
    orc = ob.Oracle(1000, 1.2, nl)
    k0, d0 = orc.extract(synth.frame(3, 0))
    k1, d1 = orc.extract(synth.frame(3, 1))
    sf, bounds = orc.tables()["scale"], (0.0, 640.0, 0.0, 480.0)
    rng = np.random.default_rng(17)
    cam = lr.camera(*lr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1]), 520.0, 520.0, 320.0, 240.0, th=th, nn_ratio=nn_ratio)
    pts = lr.make_points(rng, k1, d1, 700, cam, sf)
    bad, seen = (rng.random(700) < 0.05).astype(np.uint8), (rng.random(700) < 0.05).astype(np.uint8)
    # the table level and the logarithm agree away from the table's entries: no tested point may have its ratio within 1e-4 of one
    PO = pts["pos"].astype(np.float64) - cam["Ow"].astype(np.float64)
    ratio = pts["max_distance"].astype(np.float64) / np.linalg.norm(PO, axis=1)
    near = (np.abs(ratio[:, None] / sf.astype(np.float64) - 1.0) < 1e-4).any(1)
    assert not near.any()  # none left out
    ur = np.where(rng.random(len(k0)) < 0.5, k0["x"] - rng.uniform(3, 30, len(k0)), -1).astype(np.float32) if stereo else None
    occupant = np.where(rng.random(len(k0)) < 0.2, rng.integers(0, 3, len(k0)), -1).astype(np.int32)  # some occupants without observations
    got = hl.search_local_points("dropin", k0, d0, ur, pts, cam, occupant, sf, bounds, bad, seen)
    want = hl.search_local_points("parent", k0, d0, ur, pts, cam, occupant, sf, bounds, bad, seen)
    print(got["n_matches"], want["n_matches"], int(want["in_view"].sum()))
    assert np.array_equal(got["in_view"], want["in_view"]) and 200 < want["in_view"].sum() < 500
    iv = want["in_view"] == 1
    assert not iv[(bad | seen) == 1].any()
    assert got["track"][iv].tobytes() == want["track"][iv].tobytes() and np.array_equal(got["level"][iv], want["level"][iv])
    assert np.array_equal(got["visible"], want["in_view"].astype(np.int32)) and np.array_equal(want["visible"], got["visible"])  # IncreaseVisible: exactly the points in view, once
    assert np.array_equal(got["match"], want["match"]) and got["n_matches"] == want["n_matches"] > 100
    assert (got["match"] == -2).sum() > 20  # untouched occupants
