"""CPU: the restatement of GetSceneFlowObj's tail and CalDyna's decision in tests/dyna_restatement.py (what amos_dyna_* is held to) on
known answers, and the amos_dyna_* / labelled-gate entry points validating their arguments before any device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import dyna_restatement as dr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import flow_oracle as fo  # noqa: E402

I34 = np.eye(3, 4, dtype=np.float32)
F_OK = [1, 50, 10, 100, 1, 40, 10, 90]


def _static(rng, n=200):
    """a static scene seen twice from the identity pose: next == pre"""
    sc = dr.scene(rng, n, moving=0.0, noise=0.0, holes=0.0, state_p=1.0, far_band=False)
    sc["nxt"] = sc["pre"].copy()
    return sc


def _run(sc, Rt, motion, lk=None, F2=None, pnp_status=(1, 10, 5, 10, 1), fmat_status=F_OK):
    F2 = np.zeros(9) if F2 is None else F2
    return dr.tail(sc["pre"], sc["nxt"], sc["state"], len(sc["pre"]), F2, fmat_status, Rt, pnp_status, sc["depth_last"], sc["depth_cur"], dr.CAM,
                   sc["Tlw"], dr.FX, dr.FY, motion, lk)


def test_pre3d_matches_the_flow_oracle():
    rng = np.random.default_rng(3)
    sc = dr.scene(rng, 300, Tlw=dr.small_pose(rng))
    s = sc["state"] != 0
    cx, cy, ifx, ify = dr.CAM
    sf = fo.scene_flow(sc["depth_last"], sc["depth_cur"], sc["pre"][s], sc["nxt"][s], cx, cy, ifx, ify, sc["Tlw"], np.eye(3, dtype=np.float32),
                       np.zeros(3, np.float32))
    Rwl, twl = dr.world_of_last(sc["Tlw"])
    for k, p in enumerate(sc["pre"][s]):
        if sf[k, 7] > 0:
            assert np.array(dr.pre3d(dr.CAM, Rwl, twl, p[0], p[1], sc["depth_last"][int(p[1]), int(p[0])]), np.float32).tobytes() == sf[k, :3].tobytes()


def test_static_scene_identity_poses():
    out = _run(_static(np.random.default_rng(1)), dr.rt_of(I34), I34)
    assert out["choice"] == 1 and out["status"] == 0
    assert out["counts"][1] == out["counts"][0] == 200
    assert np.all(out["rpe"] < 1e-3)
    assert out["counts"][2] == out["counts"][3] == 200
    assert np.array_equal(out["rwc"], np.eye(3, dtype=np.float32).reshape(-1)) and np.all(out["ow"] == 0)
    assert out["counts"][5] == 0  # no scene flow
    assert out["counts"][4] == 200  # the zero F2: dd = NaN, every tracked point is an epipolar outlier


def _one_outlier_pose(sc):
    """a PnP pose (x translation) whose error exceeds 0.4 px at exactly one point, the nearest one: Rpe ~ fx * d / z"""
    z = np.sort([sc["depth_last"][int(p[1]), int(p[0])] for p in sc["pre"]]).astype(np.float64)
    d = 0.4 * (z[0] + z[1]) / 2 / dr.FX
    P = I34.copy()
    P[0, 3] = np.float32(d)
    return P


def test_choice_tie_and_one_more_motion_inlier():
    sc = _static(np.random.default_rng(2), 8)
    far = I34.copy()
    far[0, 3] = 1.0  # every point far off
    assert _run(sc, dr.rt_of(I34), far)["choice"] == 1
    tie = _run(sc, dr.rt_of(I34), I34)  # a tie chooses PnP
    assert tie["choice"] == 1 and tie["counts"][2] == tie["counts"][3] == 8
    P = _one_outlier_pose(sc)
    out = _run(sc, dr.rt_of(P), I34)  # one more motion-model inlier: the motion model, its list and its pose
    assert out["counts"][2] == 7 and out["counts"][3] == 8 and out["choice"] == 0
    assert out["pose"].tobytes() == I34.reshape(-1).tobytes()
    assert out["rpe"].tobytes() == tie["rpe"].tobytes()
    swap = _run(sc, dr.rt_of(I34), P)
    assert swap["counts"][2] == 8 and swap["counts"][3] == 7 and swap["choice"] == 1


def test_has_lk_changes_the_scores_not_the_output():
    rng = np.random.default_rng(4)
    sc = _static(rng, 50)
    far = I34.copy()
    far[0, 3] = 1.0
    a = _run(sc, dr.rt_of(I34), I34)
    b = _run(sc, dr.rt_of(I34), I34, lk=far)  # the LK pose scores badly: the motion model wins, and is the output
    assert a["choice"] == 1 and b["choice"] == 0 and b["counts"][2] == 0
    c = _run(sc, dr.rt_of(far), far, lk=I34)  # the LK pose scores perfectly: Mod (not the LK pose) is the output
    assert c["choice"] == 1 and c["pose"].tobytes() == far.reshape(-1).tobytes()


def test_no_models_are_flagged():
    sc = _static(np.random.default_rng(5), 20)
    out = _run(sc, np.zeros(12), I34, pnp_status=(0, 0, 500, 20, 0), fmat_status=[1, 9, 9, 9, 0, 0, 0, 0])
    assert out["status"] == dr.NO_PNP | dr.NO_F2
    assert out["counts"][4] == 20 and np.all(np.isnan(out["epipolar"]))


def test_epipolar_list_under_a_true_fundamental():
    rng = np.random.default_rng(6)
    sc = dr.scene(rng, 400, moving=0.2)
    out = _run(sc, dr.rt_of(sc["T"]), sc["T"], F2=dr.fundamental_of(sc["T"]))
    s = sc["state"] != 0
    assert np.all(out["epipolar"][~s] == 0)
    assert 0 < out["counts"][4] < s.sum()
    assert out["counts"][5] > 0 and np.all(out["flow"][:, 2] > 3) and np.all(out["flow"][:, 0] >= 399)  # the far band


LABELS = np.kron(np.arange(1, 13).reshape(3, 4), np.ones((160, 160))).astype(np.float64)  # 12 superpixels of 160 x 160


def test_empty_cluster_is_nan_and_not_removed():
    ids = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5], np.int32)
    match = np.float32([[10, 10], [200, 10]])
    rm, ave, ep, st = dr.decide(match, np.float32([5, 7]), np.float32([[10, 10]]), LABELS, ids, 15)
    assert ave[0] == 6 and np.isnan(ave[1]) and np.all(np.isnan(ave[1:]))
    assert rm[0] == 1 and rm.sum() == 1 and st == 0
    rm, ave, ep, st = dr.decide(np.zeros((0, 2), np.float32), np.zeros(0, np.float32), np.float32([[10, 10]]), LABELS, ids, 15)
    assert ep[0] == 1 and rm.sum() == 0  # epipolar outliers but no Rpe: NaN >= 3 is false


def test_sum_is_sequential_float():
    ids = np.zeros(12, np.int32)
    r = np.float32([1e8, 1, -1e8, 1])  # sequential float: ((1e8 + 1) - 1e8) + 1 = 1
    rm, ave, ep, st = dr.decide(np.float32([[1, 1]] * 4), r, np.zeros((0, 2), np.float32), LABELS, ids, 15)
    assert ave[0] == np.float32(0.25)


def test_two_outliers_in_one_superpixel_count_once():
    ids = np.arange(12, dtype=np.int32) % 3
    tm = np.float32([[10, 10], [20, 30], [170, 10]])  # superpixels 1, 1, 2 -> ids 0, 0, 1
    rm, ave, ep, st = dr.decide(np.float32([[10, 10], [170, 10]]), np.float32([4, 2]), tm, LABELS, ids, 15)
    assert ep[0] == 1 and ep[1] == 1 and rm[0] == 1 and rm[1] == 0


def test_label_zero_is_skipped_and_flagged():
    labels = LABELS.copy()
    labels[:20, :20] = 0
    ids = np.zeros(12, np.int32)
    rm, ave, ep, st = dr.decide(np.float32([[5, 5], [30, 30]]), np.float32([9, 4]), np.float32([[5, 5]]), labels, ids, 15)
    assert st == dr.BAD_MATCH_LABEL | dr.BAD_TM_LABEL
    assert ave[0] == 4 and ep[0] == 0 and rm[0] == 0
    ids[3] = 99
    rm, ave, ep, st = dr.decide(np.float32([[500, 10]]), np.float32([9]), np.zeros((0, 2), np.float32), LABELS, ids, 15)
    assert st == dr.BAD_ID


def test_reset_frame_removes_nothing():
    r = dr.reset()
    rm, ave, ep, st = dr.decide(r["match"], r["rpe"], r["tm"], LABELS, np.zeros(12, np.int32), 15)
    assert rm.sum() == 0 and np.all(np.isnan(ave)) and st == 0


def test_dyna_entry_points_reject_bad_arguments(pkg):
    """amos_dyna_* and amos_orb_gate_labels_batch_device validate before touching the device (this runs without a GPU)."""
    L = pkg.lib()
    for name in ("amos_dyna_create", "amos_dyna_destroy", "amos_dyna_stream", "amos_dyna_results_device", "amos_dyna_tail_device",
                 "amos_dyna_reset_frame_device", "amos_dyna_decide_batch_device", "amos_dyna_scene_flow_obj_device", "amos_dyna_copy_to_host",
                 "amos_orb_gate_labels_batch_device"):
        assert hasattr(L, name) and name in pkg.EXPORTS
    h = C.c_void_p()
    assert L.amos_dyna_create(C.c_int(0), None, C.c_int(0), C.c_int(1), C.byref(h)) == -1 and not h.value
    assert L.amos_dyna_create(C.c_int(0), None, C.c_int(4097), C.c_int(1), C.byref(h)) == -1
    assert L.amos_dyna_create(C.c_int(0), None, C.c_int(100), C.c_int(0), C.byref(h)) == -1
    assert L.amos_dyna_create(C.c_int(0), None, C.c_int(100), C.c_int(1), None) == -1
    buf = C.c_void_p(16)
    cam = pkg.SceneFlowCamera(320.0, 240.0, 1 / 500.0, 1 / 500.0)
    poses = pkg.DynaPoses()
    d = C.c_double
    assert L.amos_dyna_tail_device(None, C.c_int(0), buf, buf, buf, buf, buf, buf, buf, buf, buf, C.c_size_t(640), buf, C.c_size_t(640), C.c_int(640),
                                   C.c_int(480), C.byref(cam), d(500), d(500), C.byref(poses)) == -1
    for fx, fy in ((float("inf"), 500.0), (500.0, float("inf")), (float("nan"), 500.0), (0.0, 500.0)):  # the PnP's camera rule: finite, positive
        assert L.amos_dyna_tail_device(None, C.c_int(0), buf, buf, buf, buf, buf, buf, buf, buf, buf, C.c_size_t(640), buf, C.c_size_t(640), C.c_int(640),
                                       C.c_int(480), C.byref(cam), d(fx), d(fy), C.byref(poses)) == -1
    assert L.amos_dyna_reset_frame_device(None, C.c_int(0)) == -1
    assert L.amos_dyna_decide_batch_device(None, C.c_int(1), buf, C.c_size_t(0), C.c_size_t(640), C.c_int(640), C.c_int(480), buf, C.c_size_t(0),
                                           C.c_int(100), C.c_int(15), buf, C.c_size_t(15)) == -1
    assert L.amos_dyna_scene_flow_obj_device(None, C.c_int(0), buf, buf, buf, buf, buf, C.c_size_t(640), buf, C.c_size_t(640), C.c_int(640),
                                             C.c_int(480), buf, C.c_size_t(640), buf, C.c_size_t(640), C.byref(cam), d(500), d(500),
                                             C.byref(poses)) == -1
    r = pkg.DynaResults()
    assert L.amos_dyna_results_device(None, C.byref(r)) == -1
    assert L.amos_dyna_copy_to_host(None, buf, buf, C.c_size_t(4)) == -1
    assert L.amos_orb_gate_labels_batch_device(None, buf, C.c_size_t(0), C.c_size_t(640), buf, C.c_size_t(0), C.c_size_t(640), buf, C.c_size_t(0),
                                               C.c_int(100), buf, C.c_size_t(15), C.c_int(15), buf) == -1
    L.amos_dyna_stream.restype = C.c_void_p
    L.amos_dyna_stream.argtypes = [C.c_void_p]
    assert L.amos_dyna_stream(None) is None
    L.amos_dyna_destroy.restype = None
    L.amos_dyna_destroy.argtypes = [C.c_void_p]
    L.amos_dyna_destroy(None)
    if L.amos_device_count() < 1:  # without a GPU: an error code, not a crash
        assert L.amos_dyna_create(C.c_int(0), None, C.c_int(100), C.c_int(1), C.byref(h)) == -2 and not h.value
        with pytest.raises(pkg.AmosError):
            pkg.SceneFlowDyna(max_points=100, max_frames=1)
