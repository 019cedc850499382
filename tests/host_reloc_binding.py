"""ctypes binding of tests/host_reloc/libamos_host_reloc_test.so: the drop-ins of amos-slam_amd/host/FrameRelocalization.h
(ORB_SLAM2::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) and ORB_SLAM2::RefineRelocalization) on the stand-in Frame /
KeyFrame / MapPoint objects that tests/host_binding.py builds for the reference-signature adaptors (test_camera, test_kf, test_points)."""
import ctypes as C
import os

import numpy as np

import host_binding as hb

SO = os.path.join(hb.ROOT, "tests", "host_reloc", "libamos_host_reloc_test.so")

_lib = None


def lib():
    global _lib
    if _lib is None:
        hb.host()  # the HIP runtime and the product libraries first
        _lib = C.CDLL(SO)
        _lib.amos_host_reloc_last_error.restype = C.c_char_p
    return _lib


def _chk(rc, what):
    if rc < 0:
        raise RuntimeError(f"{what} rc={rc}: {lib().amos_host_reloc_last_error().decode()}")
    return rc


def search_reloc(cur, kf, pts, already_found, th, orb_dist, check_ori=True, repeat=1):
    """The arguments of hb.ref_search_reloc -> (nadditional, CurrentFrame.mvpMapPoints as indices into the point table, ms per call)"""
    out = np.zeros(max(cur.n, 1), np.int32)
    af = np.ascontiguousarray(already_found, np.uint8)
    ms = C.c_double(0)
    n = _chk(lib().amos_host_reloc_search(C.byref(cur), C.byref(kf), C.byref(pts), hb._p(af), C.c_float(th), C.c_int(orb_dist),
                                          C.c_int(int(check_ori)), C.c_int(repeat), hb._p(out), C.byref(ms)), "amos_host_reloc_search")
    return n, out[:cur.n], ms.value


def refine_relocalization(cur, kf, pts, vp_matches, inliers):
    """cur: the frame with the pose PnP found in its camera; vp_matches [cur.n]: index into the point table or -1; inliers [cur.n].
    -> dict(n_good, points, outlier, Tcw [12], set_pose)"""
    vp, inl = np.ascontiguousarray(vp_matches, np.int32), np.ascontiguousarray(inliers, np.uint8)
    assert len(vp) == len(inl) == cur.n
    points, outlier = np.zeros(max(cur.n, 1), np.int32), np.zeros(max(cur.n, 1), np.uint8)
    Tcw, set_pose = np.zeros(12, np.float32), C.c_int32(0)
    n = _chk(lib().amos_host_refine_relocalization(C.byref(cur), C.byref(kf), C.byref(pts), hb._p(vp), hb._p(inl), hb._p(points), hb._p(outlier),
                                                   hb._p(Tcw), C.byref(set_pose)), "amos_host_refine_relocalization")
    return dict(n_good=n, points=points[:cur.n], outlier=outlier[:cur.n], Tcw=Tcw, set_pose=set_pose.value)
