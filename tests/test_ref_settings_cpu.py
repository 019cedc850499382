"""The reference's settings files without a GPU: the reader of tests/ref_settings.py on every file, the host-only amos_frame_image_bounds
against the CPU oracle for every case, and Frame::PosInGrid as the search restatements compute it (local_points_restatement.grid_cells)
against the oracle's at the bounds of TUM1, Bonn and EuRoC mono.  (The search restatements themselves are held to the oracle at these
bounds in tests/test_searches_at_camera_bounds_cpu.py.)"""
import numpy as np
import pytest

import local_points_restatement as lr
import ref_settings as rs

f32 = np.float32

# sensor, file -> (width, height, fx, fy, cx, cy, distortion as written, bf, ThDepth, DepthMapFactor, nFeatures, scaleFactor, nLevels, iniThFAST,
# minThFAST), typed in from the files
EXPECTED = {
    ("Monocular", "EuRoC"): (752, 480, 458.654, 457.296, 367.215, 248.375, (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05), None, None, None, 1000, 1.2, 8, 20, 7),
    ("Monocular", "KITTI00-02"): (1241, 376, 718.856, 718.856, 607.1928, 185.2157, (0.0, 0.0, 0.0, 0.0), None, None, None, 2000, 1.2, 8, 20, 7),
    ("Monocular", "KITTI03"): (1241, 376, 721.5377, 721.5377, 609.5593, 172.854, (0.0, 0.0, 0.0, 0.0), None, None, None, 2000, 1.2, 8, 20, 7),
    ("Monocular", "KITTI04-12"): (1241, 376, 707.0912, 707.0912, 601.8873, 183.1104, (0.0, 0.0, 0.0, 0.0), None, None, None, 2000, 1.2, 8, 20, 7),
    ("Monocular", "TUM1"): (640, 480, 517.306408, 516.469215, 318.643040, 255.313989, (0.262383, -0.953104, -0.005358, 0.002628, 1.163314), None, None, None, 1000, 1.2, 8, 20, 7),
    ("Monocular", "TUM2"): (640, 480, 520.908620, 521.007327, 325.141442, 249.701764, (0.231222, -0.784899, -0.003257, -0.000105, 0.917205), None, None, None, 1000, 1.2, 8, 20, 7),
    ("Monocular", "TUM3"): (640, 480, 535.4, 539.2, 320.1, 247.6, (0.0, 0.0, 0.0, 0.0), None, None, None, 1000, 1.2, 8, 20, 7),
    ("RGB-D", "Bonn"): (640, 480, 542.822841, 542.576870, 315.593520, 237.756098, (0.039903, -0.099343, -0.000730, -0.000144), 40.0, 40.0, 5000.0, 1000, 1.2, 8, 20, 7),
    ("RGB-D", "TUM1"): (640, 480, 517.306408, 516.469215, 318.643040, 255.313989, (0.262383, -0.953104, -0.005358, 0.002628, 1.163314), 40.0, 40.0, 5000.0, 1000, 1.2, 8, 20, 7),
    ("RGB-D", "TUM2"): (640, 480, 520.908620, 521.007327, 325.141442, 249.701764, (0.231222, -0.784899, -0.003257, -0.000105, 0.917205), 40.0, 40.0, 5208.0, 1000, 1.2, 8, 20, 7),
    ("RGB-D", "TUM3"): (640, 480, 535.4, 539.2, 320.1, 247.6, (0.0, 0.0, 0.0, 0.0), 40.0, 40.0, 5000.0, 1000, 1.2, 8, 20, 7),
    ("RGB-D", "realsense"): (640, 480, 913.7, 913.6, 651.7, 362.8, (0.0, 0.0, 0.0, 0.0), 40.0, 40.0, 5000.0, 1000, 1.2, 8, 20, 7),
    ("Stereo", "EuRoC"): (752, 480, 435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297, (0.0, 0.0, 0.0, 0.0), 47.90639384423901, 35.0, None, 1200, 1.2, 8, 20, 7),
    ("Stereo", "KITTI00-02"): (1241, 376, 718.856, 718.856, 607.1928, 185.2157, (0.0, 0.0, 0.0, 0.0), 386.1448, 35.0, None, 2000, 1.2, 8, 20, 7),
    ("Stereo", "KITTI03"): (1241, 376, 721.5377, 721.5377, 609.5593, 172.854, (0.0, 0.0, 0.0, 0.0), 387.5744, 40.0, None, 2000, 1.2, 8, 20, 7),
    ("Stereo", "KITTI04-12"): (1241, 376, 707.0912, 707.0912, 601.8873, 183.1104, (0.0, 0.0, 0.0, 0.0), 379.8145, 40.0, None, 2000, 1.2, 8, 12, 7),
}


def test_the_files_are_the_sixteen_of_the_three_sensor_folders():
    assert rs.files() == sorted(EXPECTED)


@pytest.mark.parametrize("sensor,name", sorted(EXPECTED))
def test_reader(sensor, name):
    s = rs.read(sensor, name)
    w, h, fx, fy, cx, cy, dist, bf, th_depth, dmf, nf, sf, nl, ini, mn = EXPECTED[(sensor, name)]
    assert (s.sensor, s.name, s.width, s.height) == (sensor, name, w, h)
    for got, want in ((s.fx, fx), (s.fy, fy), (s.cx, cx), (s.cy, cy), (s.bf, bf), (s.th_depth, th_depth), (s.depth_map_factor, dmf), (s.scale_factor, sf)):
        if want is None:
            assert got is None
        else:
            assert isinstance(got, f32) and got == f32(want)  # a float, as Tracking.cc reads it
    assert len(s.dist) == len(dist) and all(isinstance(g, f32) and g == f32(d) for g, d in zip(s.dist, dist))
    assert (s.n_features, s.n_levels, s.ini_th, s.min_th) == (nf, nl, ini, mn)
    assert "LEFT.D" not in rs.raw(sensor, name) and "rows" not in rs.raw(sensor, name)  # the matrix blocks stay unread


def test_cases_are_distinct_in_what_the_kernels_see():
    cases = rs.cases()
    keys = [rs.kernel_key(s) for s in cases]
    assert len(set(keys)) == len(keys) == 16
    # the same camera in two sensor folders is two cases: the RGB-D front end also gets bf and the depth factor
    assert rs.kernel_key(rs.read("Monocular", "TUM1"))[1:] == rs.kernel_key(rs.read("RGB-D", "TUM1"))[1:-2]
    # ThDepth reaches no kernel: a copy that differs in it alone is the same case
    a = rs.read("Stereo", "KITTI03")
    assert rs.kernel_key(a) == rs.kernel_key(a._replace(th_depth=f32(35.0)))
    assert rs.kernel_key(a) != rs.kernel_key(a._replace(ini_th=12))


@pytest.mark.parametrize("s", rs.cases(), ids=rs.case_id)
def test_host_image_bounds_equal_the_oracle(pkg, ob, s):
    got = pkg.image_bounds(s.width, s.height, *rs.intrinsics(s), rs.dist_array(s))
    want = ob.image_bounds(s.width, s.height, *rs.intrinsics(s), rs.dist_array(s))
    assert got == want
    assert (want == (0.0, float(s.width), 0.0, float(s.height))) == (s.dist[0] == 0)


def test_image_bounds_of_the_searches_cameras(ob):
    """TUM1's bounds lie inside the image, Bonn's and EuRoC's outside; none is zero-based or round."""
    b = {name: rs.search_camera(ob, name)["bounds"] for name in rs.SEARCH_CAMERAS}
    print(b)
    assert b["TUM1"][0] > 0 and b["TUM1"][2] > 0 and b["TUM1"][1] < 640 and b["TUM1"][3] < 480
    for name, (w, h) in (("Bonn", (640, 480)), ("EuRoC", (752, 480))):
        assert b[name][0] < 0 and b[name][2] < 0 and b[name][1] > w and b[name][3] > h
    for name, want in (("TUM1", (10.80, 626.05, 14.67, 473.31)), ("Bonn", (-2.62, 643.41, -1.74, 482.74)), ("EuRoC", (-135.80, 895.51, -92.88, 565.55))):
        assert np.allclose(b[name], want, atol=0.006), name
    assert all(v != round(v) for bounds in b.values() for v in bounds)


@pytest.mark.parametrize("name", list(rs.SEARCH_CAMERAS))
def test_grid_cells_equal_the_oracle_at_camera_bounds(ob, synth, name):
    """With min_x, min_y != 0 the subtraction in (x - mnMinX) * mfGridElementWidthInv rounds: the restatement's cells equal the oracle's
    on the undistorted keypoints, and differ from the cells at (0, w, 0, h)."""
    sc = rs.camera_scene(ob, synth, name, n_frames=1)
    kps, _ = sc["frames"][0]
    cell = lr.grid_cells(kps, sc["bounds"])
    h, w = int(sc["image_bounds"][3]), int(sc["image_bounds"][1])
    want = ob.rgbd_glue(kps, np.zeros((h, w), f32), 1.0, sc["bounds"], kps_un=kps)[2]
    assert np.array_equal(cell, want) and (cell >= 0).all() and len(np.unique(cell)) > 300
    assert (cell != lr.grid_cells(kps, sc["image_bounds"])).sum() > len(kps) // 10
