"""ctypes binding of tests/host_pose/libamos_host_pose_test.so: Optimizer::PoseOptimization on a stand-in Frame (with SetPose) and MapPoint
objects, through the drop-in ORB_SLAM2::PoseOptimization ("dropin") or through amos_pose_core.h compiled for the host ("core")."""
import ctypes as C
import os

import numpy as np

import host_binding as hb
import pose_optimization_restatement as pr

SO = os.path.join(hb.ROOT, "tests", "host_pose", "libamos_host_pose_test.so")

_lib = None


def lib():
    global _lib
    if _lib is None:
        hb.host()  # the HIP runtime and the product libraries first
        _lib = C.CDLL(SO)
        _lib.amos_host_pose_last_error.restype = C.c_char_p
    return _lib


def pose_optimization(which, case, outlier=None, repeat=1):
    """case: a frame of tests/pose_optimization_cases.py (count == features).  The map point of feature i is point match[i] of the case.
    -> dict(ret, outlier [n], Tcw [12], set_pose, ms)"""
    kps = np.ascontiguousarray(case["kps"], hb.KP)
    n = len(kps)
    ur = None if case["u_right"] is None else np.ascontiguousarray(case["u_right"], np.float32)
    match = np.asarray(case["match"], np.int32)
    has_point = (match >= 0).astype(np.uint8)
    idx = np.where(match >= 0, match, 0)
    world = np.ascontiguousarray(np.asarray(case["pos"], np.float32).reshape(-1, 3)[idx], np.float32)
    obs = np.asarray(case["has_obs"], bool)[idx].astype(np.int32)
    cam = np.ascontiguousarray(case["camera"], pr.CAMERA).reshape(1)
    sig = np.ascontiguousarray(case["inv_sigma2"], np.float32)
    flags = np.zeros(max(n, 1), np.uint8) if outlier is None else np.array(outlier, np.uint8)
    Tcw, set_pose, ms = np.zeros(12, np.float32), C.c_int32(0), C.c_double(0)
    ret = lib().amos_host_pose_optimization(hb._p(cam), C.c_int(n), hb._p(kps), hb._p(ur), hb._p(has_point), hb._p(world), hb._p(obs), hb._p(sig),
                                            C.c_int(len(sig)), C.c_int({"dropin": 0, "core": 1}[which]), C.c_int(repeat), hb._p(flags), hb._p(Tcw),
                                            C.byref(set_pose), C.byref(ms))
    if ret < 0:
        raise RuntimeError(f"amos_host_pose_optimization rc={ret}: {lib().amos_host_pose_last_error().decode()}")
    return dict(ret=ret, outlier=flags[:n], Tcw=Tcw, set_pose=set_pose.value, ms=ms.value)
