"""ctypes binding of tests/host_loop_points/libamos_host_loop_points_test.so: ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
through the drop-in (amos-slam_amd/host/KeyFrameLoopPoints.h) or the host class on stand-in KeyFrame / MapPoint objects, and the host
compilation of amos-slam_amd/csrc/amos_loop_points_core.h."""
import ctypes as C
import os

import numpy as np

import host_binding as hb
import loop_points_restatement as lp

SO = os.path.join(hb.ROOT, "tests", "host_loop_points", "libamos_host_loop_points_test.so")
MAX_LEVELS = 16
WHICH = {"dropin": 0, "host_class": 1}
STATS = np.dtype([(k, "<i4") for k in lp.STATS])
_lib = None


class KF(C.Structure):
    _fields_ = [("n", C.c_int32), ("keys_un", C.c_void_p), ("desc", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("n_levels", C.c_int32),
                ("scale_factors", C.c_float * MAX_LEVELS)]


def lib():
    global _lib
    if _lib is None:
        hb.host()  # the HIP runtime and the product libraries first
        _lib = C.CDLL(SO)
        _lib.amos_host_loop_points_last_error.restype = C.c_char_p
        _lib.amos_host_loop_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        _lib.amos_host_loop_points_unscale.argtypes = [C.c_void_p, C.c_void_p]
        _lib.amos_host_loop_points_unscale.restype = None
    return _lib


def standin(kps, desc, intr, scale_factors, bounds):
    """-> (KF struct, keepalive)"""
    kps, desc = np.ascontiguousarray(kps, hb.KP), np.ascontiguousarray(desc, np.uint8)
    k = KF()
    k.n, k.keys_un, k.desc = len(kps), kps.ctypes.data, desc.ctypes.data
    k.fx, k.fy, k.cx, k.cy = intr
    k.min_x, k.max_x, k.min_y, k.max_y = bounds
    k.n_levels = len(scale_factors)
    for i, s in enumerate(scale_factors):
        k.scale_factors[i] = float(s)
    return k, (kps, desc)


def search(which, k, points, Scw, row, th=10, repeat=1):
    """-> (nmatches, vpMatched on return in the row's coding, the drop-in's stats record, ms per run)"""
    pts = np.ascontiguousarray(points, lp.MAP_POINT)
    row = np.ascontiguousarray(row, np.int32)
    S = np.ascontiguousarray(Scw, np.float32).reshape(16)
    out, ms, stats = np.full(max(len(row), 1), -9, np.int32), np.zeros(max(repeat, 1)), np.zeros(1, STATS)
    rc = lib().amos_host_loop_points(C.addressof(k), hb._p(pts), len(pts), hb._p(S), hb._p(row), int(th), WHICH[which], repeat, hb._p(out), hb._p(stats),
                                     hb._p(ms))
    if rc < 0:
        raise RuntimeError(f"amos_host_loop_points rc={rc}: {lib().amos_host_loop_points_last_error().decode()}")
    return rc, out[:len(row)], stats[0], ms


def unscale(Scw):
    """The host compilation of the core header -> (Rcw [3, 3], tcw, Ow, scw)"""
    S = np.ascontiguousarray(Scw, np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    lib().amos_host_loop_points_unscale(hb._p(S), hb._p(out))
    return out[:9].reshape(3, 3), out[9:12], out[12:15], out[15]
