"""ctypes binding of tests/host_local/libamos_host_local_test.so: step 2 of Tracking::SearchLocalPoints on stand-in Frame / MapPoint objects,
through the drop-in ORB_SLAM2::SearchLocalPoints ("dropin") or through the chain the host classes had before it ("parent": isInFrustum on
the host, then ORBmatcherFor::SearchByProjection)."""
import ctypes as C
import os

import numpy as np

import host_binding as hb
import local_points_restatement as lr

SO = os.path.join(hb.ROOT, "tests", "host_local", "libamos_host_local_test.so")


class TestFrame(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
                ("Ow", C.c_float * 3), ("n_levels", C.c_int32), ("scale_factors", C.c_float * 16), ("n", C.c_int32), ("keys_un", C.c_void_p),
                ("desc", C.c_void_p), ("u_right", C.c_void_p), ("occupant_obs", C.c_void_p)]


class TestPoints(C.Structure):
    _fields_ = [("n", C.c_int32), ("world", C.c_void_p), ("normal", C.c_void_p), ("desc", C.c_void_p), ("obs", C.c_void_p), ("bad", C.c_void_p),
                ("seen", C.c_void_p), ("min_dist", C.c_void_p), ("max_dist", C.c_void_p)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        hb.host()  # the HIP runtime and the product libraries first
        _lib = C.CDLL(SO)
        _lib.amos_host_local_last_error.restype = C.c_char_p
    return _lib


def search_local_points(which, kps, desc, u_right, points, cam, occupant_obs, scale_factors, bounds, bad=None, seen=None, repeat=1):
    """points: lr.MAP_POINT records (flags bit 1 = one observation; the skip bit is ignored: pass `bad` / `seen`).  -> dict(n_matches, in_view,
    track [n x 4], level, visible, match, ms)"""
    kps, desc = np.ascontiguousarray(kps, hb.KP), np.ascontiguousarray(desc, np.uint8)
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    occ = np.ascontiguousarray(occupant_obs, np.int32)
    sf = np.asarray(scale_factors, np.float32)
    f = TestFrame()
    f.fx, f.fy, f.cx, f.cy, f.mbf = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "mbf"))
    f.min_x, f.max_x, f.min_y, f.max_y = bounds
    f.Rcw[:], f.tcw[:], f.Ow[:] = cam["Rcw"].tolist(), cam["tcw"].tolist(), cam["Ow"].tolist()
    f.n_levels = len(sf)
    for i, s in enumerate(sf):
        f.scale_factors[i] = float(s)
    f.n, f.keys_un, f.desc, f.u_right, f.occupant_obs = len(kps), kps.ctypes.data, desc.ctypes.data, None if ur is None else ur.ctypes.data, occ.ctypes.data
    m = len(points)
    world, normal = np.ascontiguousarray(points["pos"], np.float32), np.ascontiguousarray(points["normal"], np.float32)
    pdesc = np.ascontiguousarray(points["desc"], np.uint8)
    obs = ((points["flags"] & lr.HAS_OBS) != 0).astype(np.int32)
    bad = np.zeros(m, np.uint8) if bad is None else np.ascontiguousarray(bad, np.uint8)
    seen = np.zeros(m, np.uint8) if seen is None else np.ascontiguousarray(seen, np.uint8)
    mind, maxd = np.ascontiguousarray(points["min_distance"], np.float32), np.ascontiguousarray(points["max_distance"], np.float32)
    t = TestPoints(m, world.ctypes.data, normal.ctypes.data, pdesc.ctypes.data, obs.ctypes.data, bad.ctypes.data, seen.ctypes.data,
                   mind.ctypes.data, maxd.ctypes.data)
    in_view, track = np.zeros(max(m, 1), np.uint8), np.zeros((max(m, 1), 4), np.float32)
    level, visible, match = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32), np.zeros(max(len(kps), 1), np.int32)
    ms = C.c_double(0)
    n = lib().amos_host_local_points(C.byref(f), C.byref(t), C.c_float(float(cam["th"])), C.c_float(float(cam["nn_ratio"])),
                                     {"dropin": 0, "parent": 1}[which], repeat, hb._p(in_view), hb._p(track), hb._p(level), hb._p(visible),
                                     hb._p(match), C.byref(ms))
    if n < 0:
        raise RuntimeError(f"amos_host_local_points rc={n}: {lib().amos_host_local_last_error().decode()}")
    return dict(n_matches=n, in_view=in_view[:m], track=track[:m], level=level[:m], visible=visible[:m], match=match[:len(kps)], ms=ms.value)
