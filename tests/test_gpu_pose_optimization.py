"""amos_match_pose_optimization_batch_device on the GPU against the Python restatement (tests/pose_optimization_restatement.py), bit for
bit: every field of amos_pose_result, d_outlier with the bytes it must leave alone, and d_match with clear_outliers 0 and 1.  (A NaN
compares equal to a NaN: its sign and payload are the processor's, not the arithmetic's.)"""
import numpy as np
import pytest

import motion_model_restatement as mr
import pose_optimization_cases as pc
import pose_optimization_restatement as pr

pytestmark = pytest.mark.gpu

FLOAT_FIELDS = ("Rt", "Tcw", "Ow", "lambda", "chi2")
INT_FIELDS = ("n_edges", "n_inliers", "n_inliers_with_obs", "rounds", "status", "iterations", "trials")
FILL = 7  # what d_outlier holds on entry


@pytest.fixture(scope="module")
def cases():
    return pc.all_cases()


@pytest.fixture(scope="module")
def wanted(cases):
    """the restatement of every case, once: {(name, clear, with_flags): (result, outlier, match)}"""
    out = {}
    for name, c in cases.items():
        for with_flags in (False, True):
            cc = c if with_flags else dict(c, has_obs=None)
            for clear in (0, 1):
                out[name, clear, with_flags] = pc.restate(cc, clear, FILL)
    return out


def point_records(pkg, case, form):
    """the case's points as the records of `form` -> (array, stride, flags_offset, has_obs_bit)"""
    pos = case["pos"]
    if form == "xyz":
        return np.ascontiguousarray(pos, np.float32), 12, -1, 0
    dtype, bit = (pkg.MAP_POINT_DTYPE, pkg.MAP_POINT_HAS_OBS) if form == "map" else (pkg.LAST_POINT_DTYPE, pkg.LAST_POINT_HAS_OBS)
    rec = np.zeros(len(pos), dtype)
    rec["pos"] = pos
    rec["flags"] = np.where(case["has_obs"], bit, 0) | 1  # (the skip bit is the searches' business)
    return rec, dtype.itemsize, dtype.fields["flags"][1], bit


def run_device(pkg, batch, clear, form="xyz", pad=3, matcher=None, repeat=1):
    """`repeat` calls on freshly uploaded arrays -> [(results [frames], outlier [frames][cap], match [frames][cap])]"""
    import torch
    nf = len(batch)
    cap = max(len(c["kps"]) for c in batch) + pad
    kps, ur = np.zeros((nf, cap), pkg.KP_DTYPE), np.full((nf, cap), -1, np.float32)
    match, counts = np.full((nf, cap), -1, np.int32), np.zeros(nf, np.int32)
    recs = []
    for f, c in enumerate(batch):
        n = len(c["kps"])
        kps[f, :n], ur[f, :n], match[f, :n], counts[f] = c["kps"], c["u_right"], c["match"], c["count"]
        rec, stride, flags_offset, bit = point_records(pkg, c, form)
        recs.append(rec)
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)
    cams = np.array([c["camera"] for c in batch], pkg.POSE_CAMERA_DTYPE)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_kps, d_ur, d_counts, d_pts = up(kps), up(ur), up(counts), up(np.concatenate(recs))
    mt = matcher or pkg.OrbMatcher()
    out = []
    for _ in range(repeat):
        d_match = up(match)
        d_outlier = torch.full((nf, cap), FILL, dtype=torch.uint8, device="cuda")
        d_result = torch.full((nf, pkg.POSE_RESULT_DTYPE.itemsize), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        mt.pose_optimization_batch_device(d_kps.data_ptr(), d_counts.data_ptr(), d_match.data_ptr(), d_pts.data_ptr(), off, cams, cap,
                                          batch[0]["inv_sigma2"], d_outlier.data_ptr(), d_result.data_ptr(), point_stride=stride,
                                          flags_offset=flags_offset, has_obs_bit=bit, clear_outliers=clear, d_u_right=d_ur.data_ptr())
        mt.sync()
        torch.cuda.synchronize()
        out.append((np.frombuffer(d_result.cpu().numpy().tobytes(), pkg.POSE_RESULT_DTYPE), d_outlier.cpu().numpy(),
                    np.frombuffer(d_match.cpu().numpy().tobytes(), np.int32).reshape(nf, cap)))
    if matcher is None:
        mt.close()
    return out


def assert_frame(name, got, f, n, want):
    """frame f of a device call equals the restatement's (result, outlier, match)"""
    res, outlier, match = got
    w_res, w_outlier, w_match = want
    for field in FLOAT_FIELDS:
        assert pc.same_bits(res[field][f], w_res[field]), (name, field, res[field][f], w_res[field])
    for field in INT_FIELDS:
        assert np.array_equal(res[field][f], w_res[field]), (name, field, res[field][f], w_res[field])
    assert np.array_equal(outlier[f, :n], w_outlier), name
    assert (outlier[f, n:] == FILL).all(), name
    assert np.array_equal(match[f, :n], w_match) and (match[f, n:] == -1).all(), name


@pytest.mark.parametrize("form", ["xyz", "map", "last"])
@pytest.mark.parametrize("clear", [0, 1])
def test_every_case_against_the_restatement(gpu_lib, cases, wanted, clear, form):
    """all the cases as the frames of ONE call"""
    names = list(cases)
    got, = run_device(gpu_lib, [cases[k] for k in names], clear, form)
    for f, name in enumerate(names):
        w = wanted[name, clear, form != "xyz"]
        print(f"{name}: edges {got[0]['n_edges'][f]} inliers {got[0]['n_inliers'][f]} / {w[0]['n_inliers']} rounds {got[0]['rounds'][f]} "
              f"iterations {got[0]['iterations'][f]} trials {got[0]['trials'][f]}")
        assert_frame(name, got, f, len(cases[name]["kps"]), w)
    res = got[0]
    by = {name: res[f] for f, name in enumerate(names)}
    assert by["2_mono_0"]["n_inliers"] == 0 and by["2_mono_0"]["rounds"] == 0 and by["9_mixed_0"]["rounds"] == 1 and by["10_mixed_0"]["rounds"] == 4
    assert by["count_zero"]["n_edges"] == 0 and by["bad_octave"]["status"] == 1 and by["bad_match_index"]["status"] == 2
    assert tuple(by["exact_optimum"]["iterations"]) == (1, 1, 1, 1) and by["exact_optimum"]["n_inliers"] == 14   # rho == 0 terminates at once
    assert not np.isfinite(by["zero_depth_mono"]["chi2"][0])


def test_a_failed_solve(gpu_lib, wanted):
    """negative weights make H negative definite: the solve fails and tempChi is DBL_MAX until the growing lambda outweighs H"""
    c = pc.negative_sigma_case()
    for clear in (0, 1):
        got, = run_device(gpu_lib, [c], clear, "map")
        assert_frame("negative_sigma", got, 0, len(c["kps"]), pc.restate(c, clear, FILL))
    assert got[0]["trials"][0][0] > got[0]["iterations"][0][0] and got[0]["chi2"][0][0] < 0


@pytest.mark.parametrize("size", [1, 2, 33])
def test_a_frame_in_a_batch_equals_the_frame_alone(gpu_lib, cases, wanted, size):
    names = [k for k in cases if not k.startswith("2_")][5::2][:size]  # frames of different sizes
    assert len(names) == size and (size == 1 or len({len(cases[k]["kps"]) for k in names}) > 1)
    got, = run_device(gpu_lib, [cases[k] for k in names], 1, "map")
    for f, name in enumerate(names):
        assert_frame(name, got, f, len(cases[name]["kps"]), wanted[name, 1, True])
    for f in {0, size - 1}:  # the same frame alone, in another slot and capacity
        alone, = run_device(gpu_lib, [cases[names[f]]], 1, "map", pad=11)
        n = len(cases[names[f]]["kps"])
        for field in FLOAT_FIELDS + INT_FIELDS:
            assert pc.same_bits(alone[0][field][0], got[0][field][f]), (names[f], field)
        assert np.array_equal(alone[1][0, :n], got[1][f, :n]) and np.array_equal(alone[2][0, :n], got[2][f, :n])


def test_the_same_handle_twice(gpu_lib, cases, wanted):
    names = ["1000_mixed_25", "65_stereo_25", "zero_depth_mono", "300_mono_0"]
    mt = gpu_lib.OrbMatcher()
    first, second = run_device(gpu_lib, [cases[k] for k in names], 0, "last", matcher=mt, repeat=2)
    small, = run_device(gpu_lib, [cases["9_mono_25"]], 0, "last", matcher=mt)  # a smaller call on the grown scratch
    mt.close()
    for f, name in enumerate(names):
        assert_frame(name, first, f, len(cases[name]["kps"]), wanted[name, 0, True])
        assert_frame(name, second, f, len(cases[name]["kps"]), wanted[name, 0, True])
    assert_frame("9_mono_25", small, 0, len(cases["9_mono_25"]["kps"]), wanted["9_mono_25", 0, True])


def test_behind_a_motion_model_search(gpu_lib):
    """Chaining: the d_match and d_points of amos_match_motion_model_batch_device go in as they lie on the device (amos_last_point by
    stride); the result equals the restatement on the downloaded arrays."""
    import torch
    import local_points_restatement as lr
    pkg = gpu_lib
    kps, desc = mr.hand_frame(np.zeros(54, np.float32))
    rng = np.random.default_rng(11)
    n, bounds = len(kps), mr.HAND_BOUNDS
    depth = rng.uniform(0.5, 8.0, n)
    pts = np.zeros(n, mr.LAST_POINT)
    pts["pos"] = np.stack([(kps["x"] + rng.normal(0, 0.7, n) - 320.0) / 512.0 * depth, (kps["y"] + rng.normal(0, 0.7, n) - 240.0) / 512.0 * depth, depth], 1)
    pts["flags"] = np.where(rng.random(n) < 0.7, mr.HAS_OBS, 0)
    pts["desc"] = desc
    pts = pts[rng.permutation(n)[:45]]
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    mcam = mr.camera(eye, zero, eye, zero, 512.0, 512.0, 320.0, 240.0, th=7.0, retry_below=0)
    cap = n + 4
    k2, d2, cell = np.zeros((1, cap), pkg.KP_DTYPE), np.zeros((1, cap, 32), np.uint8), np.full((1, cap), -1, np.int32)
    k2[0, :n], d2[0, :n], cell[0, :n] = kps, desc, lr.grid_cells(kps, bounds)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_kps, d_desc, d_cell, d_counts, d_pts = up(k2), up(d2), up(cell), up(np.array([n], np.int32)), up(pts)
    d_start = torch.zeros((1, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_items = torch.full((1, cap), -1, dtype=torch.int32, device="cuda")
    d_query = torch.zeros((len(pts), 56), dtype=torch.uint8, device="cuda")
    d_projected = torch.zeros((len(pts),), dtype=torch.uint8, device="cuda")
    d_match = torch.full((1, cap), 12345, dtype=torch.int32, device="cuda")
    d_stats = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    d_outlier = torch.full((1, cap), FILL, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros((1, pkg.POSE_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    off = np.array([0, len(pts)], np.int32)
    mt = pkg.OrbMatcher()
    mt.grid_build_batch_device(d_cell.data_ptr(), d_counts.data_ptr(), 1, cap, d_start.data_ptr(), d_items.data_ptr())
    mt.motion_model_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), d_pts.data_ptr(),
                                 off, np.array([mcam], mr.CAMERA), cap, mr.HAND_SCALE, d_query.data_ptr(), d_projected.data_ptr(),
                                 d_match.data_ptr(), d_stats.data_ptr(), bounds=bounds)
    mt.sync()
    searched = d_match.cpu().numpy()[0, :n].copy()
    start = pc.camera(pc.rot(0.01, -0.008, 0.004), [0.01, -0.02, 0.015], 512.0, 512.0, 320.0, 240.0, 20.0)
    mt.pose_optimization_batch_device(d_kps.data_ptr(), d_counts.data_ptr(), d_match.data_ptr(), d_pts.data_ptr(), off,
                                      np.array([start], pkg.POSE_CAMERA_DTYPE), cap, pc.INV_SIGMA2, d_outlier.data_ptr(), d_result.data_ptr(),
                                      point_stride=64, flags_offset=20, has_obs_bit=pkg.LAST_POINT_HAS_OBS, clear_outliers=True)
    mt.sync()
    torch.cuda.synchronize()
    got = (np.frombuffer(d_result.cpu().numpy().tobytes(), pkg.POSE_RESULT_DTYPE), d_outlier.cpu().numpy(), d_match.cpu().numpy())
    mt.close()
    assert (searched >= 0).sum() >= 30
    want = pr.pose_optimization(kps, None, searched, pts["pos"], (pts["flags"] & mr.HAS_OBS) != 0, start, pc.INV_SIGMA2, np.full(n, FILL, np.uint8), 1)
    assert_frame("chained", got, 0, n, want)
    assert want[0]["n_inliers"] >= 30 and np.abs(want[0]["Rt"][:9].reshape(3, 3) - np.eye(3)).max() < 2e-3
