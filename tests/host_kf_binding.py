"""ctypes binding of tests/host_kf/libamos_host_kf_test.so: SearchForTriangulation and SearchByBoW(pKF1, pKF2, ...) on stand-in KeyFrame /
MapPoint objects, through the drop-ins of amos-slam_amd/host/KeyFrameSearch.h ("dropin": the batch form; "single": its single-pair form
looped) or through the host class ORBmatcherFor ("parent": one call per neighbour, as LocalMapping and LoopClosing had them)."""
import ctypes as C
import os

import numpy as np

import host_binding as hb

SO = os.path.join(hb.ROOT, "tests", "host_kf", "libamos_host_kf_test.so")
WHICH = {"dropin": 0, "parent": 1, "single": 2}
_lib = None


def lib():
    global _lib
    if _lib is None:
        hb.host()  # the HIP runtime and the product libraries first
        _lib = C.CDLL(SO)
        _lib.amos_host_kf_last_error.restype = C.c_char_p
        _lib.amos_host_kf_triangulation.argtypes = ([C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3
                                                    + [C.c_int, C.c_void_p])
        _lib.amos_host_kf_bow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float] + [C.c_int] * 3 + [C.c_void_p] * 3
    return _lib


def pose_of_neighbour(R12, t12):
    """keyframe 1 at the origin: keyframe 2's Tcw for X1 = R12 X2 + t12"""
    T = np.eye(4)
    T[:3, :3] = np.asarray(R12, np.float64).T
    T[:3, 3] = -T[:3, :3] @ np.asarray(t12, np.float64)
    return T.astype(np.float32)


def _standins(sides, K, poses, scale_factors, bad_points):
    """sides -> (TestKF structs, the point table, keepalive): feature i of side k with has_point set holds point offset_k + i; bad_points:
    (side, feature) pairs whose point isBad()"""
    kfs, keep, off = [], [], 0
    total = sum(len(s["desc"]) for s in sides)
    bad = np.zeros(max(total, 1), np.uint8)
    for k, (s, T) in enumerate(zip(sides, poses)):
        n = len(s["desc"])
        cam = hb.test_camera(T, scale_factors, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        hp = np.ones(n, bool) if s.get("has_point") is None else np.asarray(s["has_point"], bool)
        point_of = np.where(hp, off + np.arange(n), -1).astype(np.int32)
        kf, ka = hb.test_kf(cam, s["keys"], s["desc"], s.get("u_right"), point_of, s["fv"])
        kfs.append(kf)
        keep.append(ka)
        for side, feature in bad_points or ():
            if side == k:
                bad[off + feature] = 1
        off += n
    z3, z1 = np.zeros((max(total, 1), 3), np.float32), np.zeros(max(total, 1), np.float32)
    pts, kp = hb.test_points(z3, z3, np.zeros((max(total, 1), 32), np.uint8), np.ones(max(total, 1), np.int32), bad, z1, z1 + 1)
    return kfs, pts, (keep, kp), np.cumsum([0] + [len(s["desc"]) for s in sides])


def _check(rc, name):
    if rc != 0:
        raise RuntimeError(f"{name} rc={rc}: {lib().amos_host_kf_last_error().decode()}")


def triangulation(which, k1, k2s, K, poses2, f12s, scale_factors, only_stereo, check_orientation, repeat=1):
    """one keyframe 1 (at the origin) against the keyframes k2s with the poses poses2 -> dict(pairs: one [m][2] array per neighbour, returned,
    ms: wall time of each run)"""
    kfs, pts, keep, _ = _standins([k1] + list(k2s), K, [np.eye(4, dtype=np.float32)] + list(poses2), scale_factors, None)
    n2, cap = len(k2s), max(len(k1["desc"]), 1)
    ptrs = (C.c_void_p * n2)(*[C.addressof(k) for k in kfs[1:]])
    F = np.ascontiguousarray(np.stack([np.asarray(f, np.float32).reshape(9) for f in f12s]))
    pairs, counts, returned = np.zeros((n2, cap, 2), np.int32), np.zeros(n2, np.int32), np.zeros(n2, np.int32)
    ms = np.zeros(max(repeat, 1), np.float64)
    _check(lib().amos_host_kf_triangulation(C.addressof(kfs[0]), ptrs, n2, C.addressof(pts), hb._p(F), int(only_stereo), int(check_orientation),
                                            WHICH[which], repeat, hb._p(pairs), hb._p(counts), hb._p(returned), cap, hb._p(ms)),
           "amos_host_kf_triangulation")
    return dict(pairs=[pairs[k, :counts[k]].copy() for k in range(n2)], returned=returned, ms=ms)


def search_by_bow(which, k1, k2s, nn_ratio, check_orientation, bad_points=None, repeat=1):
    """-> dict(match12 [n2][n1]: the keyframe-2 FEATURE whose map point lands in vpMatches12[i] (-1: NULL), returned, ms)"""
    sides = [k1] + list(k2s)
    K, poses = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), [np.eye(4, dtype=np.float32)] * len(sides)
    kfs, pts, keep, offs = _standins(sides, K, poses, [1.0, 1.2], bad_points)
    n1, n2 = len(k1["desc"]), len(k2s)
    ptrs = (C.c_void_p * n2)(*[C.addressof(k) for k in kfs[1:]])
    m12, returned, ms = np.zeros((n2, max(n1, 1)), np.int32), np.zeros(n2, np.int32), np.zeros(max(repeat, 1), np.float64)
    _check(lib().amos_host_kf_bow(C.addressof(kfs[0]), ptrs, n2, C.addressof(pts), float(nn_ratio), int(check_orientation), WHICH[which], repeat,
                                  hb._p(m12), hb._p(returned), hb._p(ms)), "amos_host_kf_bow")
    m12 = m12[:, :n1]
    for k in range(n2):  # point index -> keyframe 2's feature
        m12[k] = np.where(m12[k] >= 0, m12[k] - offs[k + 1], -1)
    return dict(match12=m12, returned=returned, ms=ms)
