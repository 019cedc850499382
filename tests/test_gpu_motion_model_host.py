"""ORB_SLAM2::SearchByMotionModel (amos-slam_amd/host/FrameMotionModel.h) on stand-in Frame / MapPoint objects through tests/host_motion/:
equal to the chain Tracking::TrackWithMotionModel had before it -- fill, ORBmatcherFor::SearchByProjection(CurrentFrame, LastFrame, th,
bMono) (host projection, host enumeration, one distance call, host greedy loop and histogram), and again with 2 * th below 20 matches --
in its return value and in every mvpMapPoints[i]."""
import numpy as np
import pytest

import motion_model_restatement as mr

pytestmark = pytest.mark.gpu

CASES = {"sideways": (mr.MOTIONS["sideways"], 0), "forward": (mr.MOTIONS["forward"], mr.FORWARD), "retry": (dict(ry=30.0 / 520.0), 0)}  # the yaw moves every projection about 30 px


@pytest.mark.parametrize("junk", [False, True])
@pytest.mark.parametrize("case,stereo,th", [("sideways", True, 7.0), ("sideways", False, 15.0), ("forward", True, 7.0), ("retry", True, 7.0)])
def test_dropin_equals_the_host_chain(gpu_lib, ob, synth, case, stereo, th, junk):
    import host_motion_binding as hm
    orc = ob.Oracle(1000, 1.2, 8)
    k0, d0 = orc.extract(synth.frame(3, 0))
    k1, d1 = orc.extract(synth.frame(3, 1))
    sf, bounds, intr = orc.tables()["scale"], (0.0, 640.0, 0.0, 480.0), (520.0, 520.0, 320.0, 240.0)
    rng = np.random.default_rng(17)
    last = mr.pose(0.01, -0.02, 0.005, [0.05, -0.02, 0.1])
    motion, flags = CASES[case]
    cam = mr.camera(*mr.moved(last, **motion), *last, *intr, th=th, retry_below=20)
    assert mr.motion_flags(cam) == flags
    # one last-frame point per last-frame feature, as LastFrame.mvpMapPoints holds them (no replacement here: index i is feature i)
    pts = mr.make_last_points(rng, k1, d1, len(k1), last, intr, replace=False)
    ur = np.where(rng.random(len(k0)) < 0.5, k0["x"] - rng.uniform(0, 20, len(k0)), -1).astype(np.float32) if stereo else None
    occupants = np.where(rng.random(len(k0)) < 0.3, rng.integers(0, 3, len(k0)), -1).astype(np.int32) if junk else None
    got = hm.search_motion_model("dropin", k0, d0, ur, k1, pts, cam, sf, bounds, occupants)
    want = hm.search_motion_model("parent", k0, d0, ur, k1, pts, cam, sf, bounds, occupants)
    res = mr.search_motion_model(k0, d0, ur, pts, cam, sf, bounds)
    print(case, got["n_matches"], want["n_matches"], res["n_matches"], res["n_first"], res["pass"])
    assert got["n_matches"] == want["n_matches"] == res["n_matches"] and np.array_equal(got["match"], want["match"])
    assert np.array_equal(got["match"], res["match"]) and (got["match"] != -2).all()  # no occupant survives the call
    assert res["pass"] == (2 if case == "retry" else 1) and res["n_matches"] >= 20
