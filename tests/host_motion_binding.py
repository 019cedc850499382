"""ctypes binding of tests/host_motion/libamos_host_motion_test.so: the search of Tracking::TrackWithMotionModel on stand-in Frame / MapPoint
objects, through the drop-in ORB_SLAM2::SearchByMotionModel ("dropin") or through the chain Tracking had before it ("parent": fill,
ORBmatcherFor::SearchByProjection(CurrentFrame, LastFrame, th, bMono), and again with 2 * th below 20 matches)."""
import ctypes as C
import os

import numpy as np

import host_binding as hb
import motion_model_restatement as mr

SO = os.path.join(hb.ROOT, "tests", "host_motion", "libamos_host_motion_test.so")

_lib = None


def lib():
    global _lib
    if _lib is None:
        hb.host()  # the HIP runtime and the product libraries first
        _lib = C.CDLL(SO)
        _lib.amos_host_motion_last_error.restype = C.c_char_p
    return _lib


def _tcw(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = np.asarray(R, np.float32).reshape(3, 3), t
    return T


def search_motion_model(which, kps, desc, u_right, last_kps, points, cam, scale_factors, bounds, junk=None, repeat=1):
    """points: mr.LAST_POINT records, one per feature of the last frame (`last_kps`; flags: skip = no map point, bit 1 = one observation);
    cam: an mr.CAMERA record (th_retry and retry_below are Tracking's own 2 * th and 20 in both chains); junk: per current feature -1, or
    the observation count of an occupant that sits in mvpMapPoints on entry.  -> dict(n_matches, match, ms)"""
    kps, desc = np.ascontiguousarray(kps, hb.KP), np.ascontiguousarray(desc, np.uint8)
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    sf = np.asarray(scale_factors, np.float32)
    kw = dict(fx=float(cam["fx"]), fy=float(cam["fy"]), cx=float(cam["cx"]), cy=float(cam["cy"]), mb=float(cam["mb"]), mbf=float(cam["mbf"]),
              bounds=tuple(float(b) for b in bounds))
    cur_cam = hb.test_camera(_tcw(cam["Rcw"], cam["tcw"]), sf, **kw)
    last_cam = hb.test_camera(_tcw(cam["Rlw"], cam["tlw"]), sf, **kw)
    m = len(points)
    lk = np.zeros(m, hb.KP)
    lk[:] = np.ascontiguousarray(last_kps, hb.KP)
    lk["octave"], lk["angle"] = points["octave"], points["angle"]
    has_point = ((points["flags"] & mr.SKIP) == 0).astype(np.uint8)
    outlier = np.zeros(m, np.uint8)
    world, pdesc = np.ascontiguousarray(points["pos"], np.float32), np.ascontiguousarray(points["desc"], np.uint8)
    obs = ((points["flags"] & mr.HAS_OBS) != 0).astype(np.int32)
    jk = None if junk is None else np.ascontiguousarray(junk, np.int32)
    match = np.zeros(max(len(kps), 1), np.int32)
    ms = C.c_double(0)
    n = lib().amos_host_motion_model(C.byref(cur_cam), C.c_int(len(kps)), hb._p(kps), hb._p(desc), hb._p(ur), hb._p(jk), C.byref(last_cam),
                                     C.c_int(m), hb._p(lk), hb._p(lk), hb._p(has_point), hb._p(outlier), hb._p(world), hb._p(pdesc), hb._p(obs),
                                     C.c_float(float(cam["th"])), C.c_int(int(cam["mono"])), C.c_int({"dropin": 0, "parent": 1}[which]),
                                     C.c_int(repeat), hb._p(match), C.byref(ms))
    if n < 0:
        raise RuntimeError(f"amos_host_motion_model rc={n}: {lib().amos_host_motion_last_error().decode()}")
    return dict(n_matches=n, match=match[:len(kps)], ms=ms.value)
