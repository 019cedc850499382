"""ctypes binding of tests/host_sim3_optimize/libamos_host_sim3_optimize_test.so: ORB_SLAM2::OptimizeSim3
(amos-slam_amd/host/KeyFrameSim3Optimize.h) on stand-in KeyFrame / MapPoint / Sim3 objects ("dropin"), and the host compilation of
amos-slam_amd/csrc/amos_sim3_opt_core.h on one thread ("core")."""
import ctypes as C
import os

import numpy as np

import host_binding as hb
import sim3_optimization_restatement as so

SO = os.path.join(hb.ROOT, "tests", "host_sim3_optimize", "libamos_host_sim3_optimize_test.so")
BAD = 4  # a flag of the harness beside AMOS_SIM3_POINT_SKIP: the feature has a point, and it isBad()
_lib = None


class Camera(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class KF(C.Structure):
    _fields_ = [("n", C.c_int32), ("keys_un", C.c_void_p), ("points", C.c_void_p), ("cam", Camera)]


def lib():
    global _lib
    if _lib is None:
        hb.host()  # the HIP runtime and the product libraries first
        _lib = C.CDLL(SO)
        _lib.amos_host_sim3_optimize_last_error.restype = C.c_char_p
        _lib.amos_host_sim3_optimize_exp.restype = C.c_double
        _lib.amos_host_sim3_optimize_exp.argtypes = [C.c_double]
        _lib.amos_host_sim3_optimize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def exp_(x):
    return float(lib().amos_host_sim3_optimize_exp(float(x)))


def standin(kps, pts, cam):
    kps, pts = np.ascontiguousarray(kps, hb.KP), np.ascontiguousarray(pts, so.POINT)
    cam = np.ascontiguousarray(cam, so.CAMERA).reshape(1)
    k = KF()
    k.n, k.keys_un, k.points = len(kps), kps.ctypes.data, pts.ctypes.data
    C.memmove(C.addressof(k.cam), cam.ctypes.data, C.sizeof(Camera))
    return k, (kps, pts, cam)


def optimize(which, sc, inv_sigma2, repeat=1):
    """sc: a scene of tests/sim3_optimization_cases.py -> dict(ret, row, sim3 [8], result, ms).  row: "core": the row on return; "dropin": 1
    where vpMatches1 is non-NULL on return."""
    k1, keep1 = standin(sc["kps1"], sc["pts1"], sc["cam1"])
    k2, keep2 = standin(sc["kps2"], sc["pts2"], sc["cam2"])
    row = np.ascontiguousarray(sc["row"], np.int32)
    pair = np.ascontiguousarray(sc["pair"], so.PAIR).reshape(1)
    sig = np.ascontiguousarray(inv_sigma2, np.float32)
    out, sim3, res, ms = np.full(max(len(row), 1), -9, np.int32), np.zeros(8), np.zeros(1, so.RESULT), np.zeros(max(repeat, 1))
    rc = lib().amos_host_sim3_optimize(C.addressof(k1), C.addressof(k2), hb._p(row), hb._p(pair), hb._p(sig), len(sig), {"dropin": 0, "core": 1}[which],
                                       repeat, hb._p(out), hb._p(sim3), hb._p(res), hb._p(ms))
    if rc < 0:
        raise RuntimeError(f"amos_host_sim3_optimize rc={rc}: {lib().amos_host_sim3_optimize_last_error().decode()}")
    return dict(ret=rc, row=out[:len(row)], sim3=sim3, result=res[0], ms=ms)
