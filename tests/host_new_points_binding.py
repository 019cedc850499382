"""ctypes binding of tests/host_new_points/libamos_host_new_points_test.so: the host compilation of
amos-slam_amd/csrc/amos_new_points_core.h (its functions, and the complete loop over pairs and matches on the arrays of
amos_match_new_points_batch_device), and ORB_SLAM2::CreateNewMapPointCandidates (amos-slam_amd/host/KeyFrameNewPoints.h) on stand-in
KeyFrame objects ("dropin") beside what the mapping thread ran before it ("parent": the drop-in search for all neighbours, then the
host-compiled core looped over neighbours and matches)."""
import ctypes as C
import os

import numpy as np

import host_binding as hb
import kf_search_cases as kc
import new_points_restatement as nr

SO = os.path.join(hb.ROOT, "tests", "host_new_points", "libamos_host_new_points_test.so")
WHICH = {"dropin": 0, "parent": 1}
f32 = np.float32
_lib = None


class Input(C.Structure):
    """new_points_host::Input (tests/host_new_points/new_points_host.h)."""
    _fields_ = [("kps", C.c_void_p), ("kps_raw", C.c_void_p), ("counts", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p),
                ("cameras", C.c_void_p), ("pairs_1", C.c_void_p), ("pairs_2", C.c_void_p), ("match12", C.c_void_p), ("enabled", C.c_void_p),
                ("scale", C.c_void_p), ("sigma2", C.c_void_p), ("n_frames", C.c_int32), ("n_pairs", C.c_int32), ("capacity", C.c_int32),
                ("n_levels", C.c_int32)]


def lib():
    global _lib
    if _lib is None:
        hb.host()  # the HIP runtime and the product libraries first
        _lib = C.CDLL(SO)
        _lib.amos_host_new_points_last_error.restype = C.c_char_p
        _lib.amos_host_new_points_geometry.argtypes = [C.c_void_p] * 3
        _lib.amos_host_new_points_cos_stereo.argtypes = [C.c_float, C.c_float]
        _lib.amos_host_new_points_cos_stereo.restype = C.c_float
        _lib.amos_host_new_points_jacobi.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib.amos_host_new_points_jacobi.restype = None
        _lib.amos_host_new_points_null_vector.argtypes = [C.c_void_p, C.c_void_p]
        _lib.amos_host_new_points_null_vector.restype = None
        _lib.amos_host_new_points_dehomogenise.argtypes = [C.c_void_p, C.c_void_p]
        _lib.amos_host_new_points_scale_gate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.amos_host_new_points_core.argtypes = [C.c_void_p] * 4
        _lib.amos_host_new_points_core.restype = None
        _lib.amos_host_new_points_dropin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_int, C.c_void_p]
    return _lib


# ---------------------------------------------------------------------------------------------------------------- the core's functions

def geometry(c1, c2):
    c1, c2 = np.ascontiguousarray(c1, nr.KF_CAMERA).reshape(1), np.ascontiguousarray(c2, nr.KF_CAMERA).reshape(1)
    g = np.zeros(1, nr.GEOMETRY)
    return g[0], lib().amos_host_new_points_geometry(hb._p(c1), hb._p(c2), hb._p(g)) == 1


def cos_stereo(mb, d):
    return f32(lib().amos_host_new_points_cos_stereo(float(f32(mb)), float(f32(d))))


def jacobi(S, which):
    """which: "unrolled" (jacobi_sym4) or "generic" (pnp::jacobi_sym) -> (what the sweeps leave of S, V)"""
    S, V = np.array(S, np.float64).reshape(16), np.zeros(16, np.float64)
    lib().amos_host_new_points_jacobi(hb._p(S), hb._p(V), {"unrolled": 0, "generic": 1}[which])
    return S.reshape(4, 4), V.reshape(4, 4)


def null_vector(A):
    A, v = np.ascontiguousarray(A, f32).reshape(16), np.zeros(4, f32)
    lib().amos_host_new_points_null_vector(hb._p(A), hb._p(v))
    return v


def dehomogenise(v):
    v, X = np.ascontiguousarray(v, f32).reshape(4), np.zeros(3, f32)
    return X if lib().amos_host_new_points_dehomogenise(hb._p(v), hb._p(X)) else None


def scale_gate(c1, c2, o1, o2, scale, X):
    c1, c2 = np.ascontiguousarray(c1, nr.KF_CAMERA).reshape(1), np.ascontiguousarray(c2, nr.KF_CAMERA).reshape(1)
    scale, X = np.ascontiguousarray(scale, f32), np.ascontiguousarray(X, f32).reshape(3)
    return lib().amos_host_new_points_scale_gate(hb._p(c1), hb._p(c2), int(o1), int(o2), hb._p(scale), hb._p(X))


# ---------------------------------------------------------------------------------------------------------------- the arrays of the batch entry

POISON_NEW = (-7, -7, 1.5, 2.5, 3.5, -7)


def pack(case, pad=5, with_raw=True, with_right=True):
    """a case of new_points_cases.py as the [frames][capacity] arrays of amos_match_new_points_batch_device, with padding that must not be
    read as data -> dict of numpy arrays (kps_raw / u_right / depth: None when the case has none or they are switched off)"""
    sides, pairs = case["sides"], case["pairs"]
    ns, cap = len(sides), max(max(len(s["keys"]) for s in sides), 1) + pad
    any_raw = with_raw and any(s.get("keys_raw") is not None for s in sides)
    any_right = with_right and any(s.get("u_right") is not None for s in sides)
    a = dict(kps=np.zeros((ns, cap), kc.KP), counts=np.zeros(ns, np.int32), kps_raw=np.zeros((ns, cap), kc.KP) if any_raw else None,
             u_right=np.full((ns, cap), 3.0, f32) if any_right else None, depth=np.full((ns, cap), 0.25, f32) if any_right else None)
    a["kps"]["octave"] = 99
    for k, s in enumerate(sides):
        n = len(s["keys"])
        a["counts"][k] = n
        a["kps"][k, :n] = s["keys"]
        if any_raw:
            a["kps_raw"][k, :n] = s["keys_raw"] if s.get("keys_raw") is not None else s["keys"]
        if any_right:
            a["u_right"][k, :n] = s["u_right"] if s.get("u_right") is not None else -1.0
            if s.get("depth") is not None:
                a["depth"][k, :n] = s["depth"]
    a["match"] = np.full((len(pairs), cap), 31, np.int32)  # (beyond keyframe 1's count: never read)
    for p, ((s1, _), row) in enumerate(zip(pairs, case["match"])):
        a["match"][p, :len(row)] = row
    a["cams"] = np.ascontiguousarray(np.stack(case["cams"]), nr.KF_CAMERA)
    a["pairs"] = np.array(pairs, np.int32).reshape(-1, 2)
    a["enabled"] = None if case.get("enabled") is None else np.ascontiguousarray(case["enabled"], np.uint8)
    a["scale"], a["sigma2"] = (np.ascontiguousarray(x, f32) for x in case["levels"])
    a["capacity"] = cap
    return a


def stripped(case, with_raw=True, with_right=True):
    """the case as the restatement must see it when the optional arrays are switched off"""
    sides = [dict(s, keys_raw=s.get("keys_raw") if with_raw else None, u_right=s.get("u_right") if with_right else None) for s in case["sides"]]
    return dict(case, sides=sides)


def core(a):
    """new_points_host::run on packed arrays -> (new [pairs][capacity] with poison beyond n_new, verdict [pairs][capacity], stats [pairs])"""
    p1, p2 = np.ascontiguousarray(a["pairs"][:, 0]), np.ascontiguousarray(a["pairs"][:, 1])
    inp = Input(hb._p(a["kps"]), hb._p(a["kps_raw"]), hb._p(a["counts"]), hb._p(a["u_right"]), hb._p(a["depth"]), hb._p(a["cams"]), hb._p(p1),
                hb._p(p2), hb._p(a["match"]), hb._p(a["enabled"]), hb._p(a["scale"]), hb._p(a["sigma2"]), len(a["cams"]), len(p1), a["capacity"],
                len(a["scale"]))
    new = np.full((len(p1), a["capacity"]), np.array(POISON_NEW, nr.NEW_POINT), nr.NEW_POINT)
    verdict, stats = np.full((len(p1), a["capacity"]), 77, np.int32), np.zeros(len(p1), nr.NEW_POINTS_STATS)
    lib().amos_host_new_points_core(C.addressof(inp), hb._p(new), hb._p(verdict), hb._p(stats))
    return new, verdict, stats


def expected(case, cap):
    """the restatement's result in the layout of the batch entry's outputs"""
    res = nr.new_points(case["sides"], case["cams"], case["pairs"], case["match"], case["levels"], case.get("enabled"))
    new = np.full((len(res), cap), np.array(POISON_NEW, nr.NEW_POINT), nr.NEW_POINT)
    verdict, stats = np.full((len(res), cap), -1, np.int32), np.zeros(len(res), nr.NEW_POINTS_STATS)
    for p, (rows, v, st) in enumerate(res):
        new[p, :len(rows)], verdict[p, :len(v)], stats[p] = rows, v, st
    return new, verdict, stats


def write_case_file(path, a):
    """the case file of tests/host_new_points/new_points_core_main.cc"""
    with open(path, "wb") as f:
        f.write(np.array([len(a["cams"]), len(a["pairs"]), a["capacity"], len(a["scale"]), a["kps_raw"] is not None, a["u_right"] is not None,
                          a["enabled"] is not None], np.int32).tobytes())
        parts = [a["kps"], a["kps_raw"], a["counts"], a["u_right"], a["depth"], a["cams"], np.ascontiguousarray(a["pairs"][:, 0]),
                 np.ascontiguousarray(a["pairs"][:, 1]), a["match"], a["enabled"], a["scale"], a["sigma2"]]
        for part in parts:
            if part is not None:
                f.write(np.ascontiguousarray(part).tobytes())


# ---------------------------------------------------------------------------------------------------------------- the drop-in

def pose_of(cam):
    T = np.eye(4, dtype=f32)
    T[:3, :3], T[:3, 3] = cam["Rcw"].reshape(3, 3), cam["tcw"]
    return T


def dropin(which, case, check_orientation=False, repeat=1):
    """keyframe slot 0 of the case against every other slot, in order -> (return value, one NEW_POINT array per neighbour, stats or None, ms);
    raises RuntimeError with the library's text when it refuses"""
    sides, cams, (sf, _) = case["sides"], case["cams"], case["levels"]
    kfs, keep, depths = [], [], []
    for s, cam in zip(sides, cams):
        tc = hb.test_camera(pose_of(cam), sf, float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), float(cam["mb"]), float(cam["mbf"]))
        hp = np.zeros(len(s["keys"]), bool) if s.get("has_point") is None else np.asarray(s["has_point"], bool)
        raw = s["keys_raw"] if s.get("keys_raw") is not None else s["keys"]
        kf, ka = hb.test_kf(tc, raw, s["desc"], s.get("u_right"), np.where(hp, 0, -1).astype(np.int32), s["fv"], keys_un=s["keys"])
        d = None if s.get("depth") is None else np.ascontiguousarray(s["depth"], f32)
        kfs.append(kf)
        keep.append((ka, d))
        depths.append(d)
    n2, cap = len(sides) - 1, max(len(sides[0]["keys"]), 1)
    ptrs = (C.c_void_p * max(n2, 1))(*[C.addressof(k) for k in kfs[1:]])
    dptr = (C.c_void_p * (n2 + 1))(*[None if d is None else d.ctypes.data for d in depths])
    out, counts, stats = np.zeros((n2, cap), nr.NEW_POINT), np.zeros(n2, np.int32), np.zeros(n2, nr.NEW_POINTS_STATS)
    ms = np.zeros(max(repeat, 1), np.float64)
    rc = lib().amos_host_new_points_dropin(C.addressof(kfs[0]), ptrs, n2, dptr, int(check_orientation), WHICH[which], repeat, hb._p(out), hb._p(counts),
                                           hb._p(stats), cap, hb._p(ms))
    if rc < 0:
        raise RuntimeError(f"amos_host_new_points_dropin rc={rc}: {lib().amos_host_new_points_last_error().decode()}")
    return rc, [out[k, :counts[k]].copy() for k in range(n2)], stats if which == "dropin" else None, ms
