"""tests/host_sim3_binding.py -- ctypes binding of tests/host_sim3/libamos_host_sim3_test.so (built by build()): the host-compiled
single-threaded Sim3Solver over amos_sim3_core.h's pieces, and ORB_SLAM2::DeviceSim3Solver on stand-in objects."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "host_sim3", "libamos_host_sim3_test.so")
_lib = None
_v, _i, _d = C.c_void_p, C.c_int, C.c_double


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run build() of __graft_entry__.py")
        L = C.CDLL(LIB_PATH)
        L.amos_host_sim3_last_error.restype = C.c_char_p
        L.amos_host_sim3_solver_create.restype = _v
        L.amos_host_sim3_solver_create.argtypes = (_v, _v, _i, _v, _v, _i, _v, _v, _v, _i, _v)
        L.amos_host_sim3_solver_destroy.restype = None
        L.amos_host_sim3_solver_destroy.argtypes = (_v,)
        L.amos_host_sim3_solver_iterate.restype = _i
        L.amos_host_sim3_solver_iterate.argtypes = (_v, _i, _v, _v, _v, _v)
        L.amos_host_sim3_parameters.restype = _i
        L.amos_host_sim3_parameters.argtypes = (_i, _d, _i, _i)
        L.amos_host_sim3_draw3.restype = None
        L.amos_host_sim3_draw3.argtypes = (_v, _i, _v)
        L.amos_host_sim3_dropin.restype = _i
        L.amos_host_sim3_dropin.argtypes = (_v, _i, _v, _i, _v, _v, _i, _v, _v, _v, _i, _v, _v, _v, _v, _i, _v, _v, _i, _v, _d, _i, _i, _i, _i,
                                            _v, _v, _v, _v, _v, _v, _v, _v, _v, _v, _v)
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def cameras_of(pkg, pair):
    cams = np.zeros(2, pkg.SIM3_CAMERA_DTYPE)
    for k, c in enumerate((pair["cam1"], pair["cam2"])):
        for f in pkg.SIM3_CAMERA_DTYPE.names:
            cams[f][k] = c[f]
    return cams


class HostSolver:
    """The host-compiled solver: constructor + SetRansacParameters from one SIM3_PARAMS_DTYPE record, then iterate(n)."""

    def __init__(self, pkg, kps1, points1, kps2, points2, cameras, match12, level_sigma2, params):
        self.pkg = pkg
        self.kps1, self.kps2 = np.ascontiguousarray(kps1, pkg.KP_DTYPE), np.ascontiguousarray(kps2, pkg.KP_DTYPE)
        p1, p2 = np.ascontiguousarray(points1, pkg.SIM3_POINT_DTYPE), np.ascontiguousarray(points2, pkg.SIM3_POINT_DTYPE)
        cams = np.ascontiguousarray(cameras, pkg.SIM3_CAMERA_DTYPE).reshape(2)
        m12 = np.ascontiguousarray(match12, np.int32)
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        par = np.ascontiguousarray(params, pkg.SIM3_PARAMS_DTYPE).reshape(1)
        self.h = lib().amos_host_sim3_solver_create(_p(self.kps1), _p(p1), len(self.kps1), _p(self.kps2), _p(p2), len(self.kps2), _p(cams), _p(m12),
                                                    _p(sig), len(sig), _p(par))
        if not self.h:
            raise RuntimeError(lib().amos_host_sim3_last_error().decode())

    def iterate(self, n_iterations):
        """-> (result record, inlier [n1], match_out [n1], generator state)."""
        n1 = len(self.kps1)
        result = np.zeros(1, self.pkg.SIM3_RESULT_DTYPE)
        inlier, match_out = np.zeros(max(n1, 1), np.uint8), np.full(max(n1, 1), -77, np.int32)
        rng = np.zeros(1, np.uint64)
        rc = lib().amos_host_sim3_solver_iterate(self.h, n_iterations, _p(result), _p(inlier), _p(match_out), _p(rng))
        if rc != 0:
            raise RuntimeError(lib().amos_host_sim3_last_error().decode())
        return result[0], inlier[:n1], match_out[:n1], int(rng[0])

    def close(self):
        if self.h:
            lib().amos_host_sim3_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def draw3(state, N):
    """-> (three indices, the generator state behind them) from amos_sim3_core.h's sim3_draw3."""
    rng = np.array([state], np.uint64)
    idx = np.zeros(3, np.int32)
    lib().amos_host_sim3_draw3(_p(rng), N, _p(idx))
    return [int(i) for i in idx], int(rng[0])


def parameters(N, probability, min_inliers, max_iterations):
    return int(lib().amos_host_sim3_parameters(N, probability, min_inliers, max_iterations))


def dropin(pkg, objects, level_sigma2, fix_scale, seed, params, n_iterations, n_calls):
    """ORB_SLAM2::DeviceSim3Solver on stand-ins.  objects: dict(kps1, kps2, cameras [2], world1, bad1, index1, kf_points1, world2, bad2,
    index2, kf_points2, matched12) -> (dict(keys1, points1, points2, match12): the constructor's arrays; list of dict(T12 [16], has_sim3,
    no_more, n_inliers, inliers [n1], R [9], t [3], s) per call; mean ms).  n_calls = 0 runs the constructor only (no GPU)."""
    o = objects
    kps1, kps2 = np.ascontiguousarray(o["kps1"], pkg.KP_DTYPE), np.ascontiguousarray(o["kps2"], pkg.KP_DTYPE)
    cams = np.ascontiguousarray(o["cameras"], pkg.SIM3_CAMERA_DTYPE).reshape(2)
    sig = np.ascontiguousarray(level_sigma2, np.float32)
    n1, n2 = len(kps1), len(kps2)
    arr = {}
    for k in ("1", "2"):
        arr["world" + k] = np.ascontiguousarray(o["world" + k], np.float32).reshape(-1, 3)
        arr["bad" + k] = np.ascontiguousarray(o["bad" + k], np.uint8)
        arr["index" + k] = np.ascontiguousarray(o["index" + k], np.int32)
        arr["kf_points" + k] = np.ascontiguousarray(o["kf_points" + k], np.int32)
    matched = np.ascontiguousarray(o["matched12"], np.int32)
    keys1_out, points1_out = np.zeros(max(n1, 1), pkg.KP_DTYPE), np.zeros(max(n1, 1), pkg.SIM3_POINT_DTYPE)
    points2_out, match12_out = np.zeros(max(n2, 1), pkg.SIM3_POINT_DTYPE), np.zeros(max(n1, 1), np.int32)
    nc = max(n_calls, 1)
    T12, Rts = np.zeros((nc, 16), np.float32), np.zeros((nc, 13), np.float32)
    has, no_more, n_inl = (np.zeros(nc, np.int32) for _ in range(3))
    inl = np.zeros(nc * max(n1, 1), np.uint8)
    ms = C.c_double(0.0)
    sd = np.array([seed], np.uint64)
    rc = lib().amos_host_sim3_dropin(_p(kps1), n1, _p(kps2), n2, _p(cams), _p(sig), len(sig), _p(arr["world1"]), _p(arr["bad1"]), _p(arr["index1"]),
                                     len(arr["world1"]), _p(arr["kf_points1"]), _p(arr["world2"]), _p(arr["bad2"]), _p(arr["index2"]),
                                     len(arr["world2"]), _p(arr["kf_points2"]), _p(matched), int(fix_scale), _p(sd), params["probability"],
                                     params["min_inliers"], params["max_iterations"], n_iterations, n_calls, _p(keys1_out), _p(points1_out),
                                     _p(points2_out), _p(match12_out), _p(T12), _p(has), _p(no_more), _p(n_inl), _p(inl), _p(Rts), C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"amos_host_sim3_dropin rc={rc}: {lib().amos_host_sim3_last_error().decode()}")
    built = dict(keys1=keys1_out[:n1], points1=points1_out[:n1], points2=points2_out[:n2], match12=match12_out[:n1])
    inliers = inl[:n_calls * n1].reshape(n_calls, n1)
    calls = [dict(T12=T12[c], has_sim3=int(has[c]), no_more=int(no_more[c]), n_inliers=int(n_inl[c]), inliers=inliers[c], R=Rts[c, :9],
                  t=Rts[c, 9:12], s=Rts[c, 12]) for c in range(n_calls)]
    return built, calls, ms.value
