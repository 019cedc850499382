"""tests/host_reloc_pnp_binding.py -- ctypes binding of tests/host_reloc_pnp/libamos_host_reloc_pnp_test.so (built by build()): the
host-compiled single-threaded PnPsolver over amos_pnp_core.h's solver pieces, and ORB_SLAM2::DevicePnPsolver on stand-in objects."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "host_reloc_pnp", "libamos_host_reloc_pnp_test.so")
_lib = None
_v, _i, _f, _d = C.c_void_p, C.c_int, C.c_float, C.c_double


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run build() of __graft_entry__.py")
        L = C.CDLL(LIB_PATH)
        L.amos_host_reloc_pnp_last_error.restype = C.c_char_p
        L.amos_host_pnp_solver_create.restype = _v
        L.amos_host_pnp_solver_create.argtypes = (_v, _i, _v, _v, _i, _v, _i, _v)
        L.amos_host_pnp_solver_destroy.restype = None
        L.amos_host_pnp_solver_destroy.argtypes = (_v,)
        L.amos_host_pnp_solver_iterate.restype = _i
        L.amos_host_pnp_solver_iterate.argtypes = (_v, _i, _v, _v, _v)
        L.amos_host_pnp_draw4.restype = None
        L.amos_host_pnp_draw4.argtypes = (_v, _i, _v)
        L.amos_host_pnp_parameters.restype = None
        L.amos_host_pnp_parameters.argtypes = (_i, _d, _i, _i, _f, _v, _v, _v)
        L.amos_host_pnp_dropin.restype = _i
        L.amos_host_pnp_dropin.argtypes = (_v, _i, _f, _f, _f, _f, _v, _i, _v, _v, _i, _v, C.c_uint64, _d, _i, _i, _f, _f, _i, _i, _v, _v, _v, _v,
                                           _v, _v)
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class HostSolver:
    """The host-compiled solver: constructor + SetRansacParameters from one RELOC_PNP_PARAMS_DTYPE record, then iterate(n)."""

    def __init__(self, pkg, kps, bow_match, points, level_sigma2, params):
        self.pkg = pkg
        self.kps = np.ascontiguousarray(kps, pkg.KP_DTYPE)
        bow = np.ascontiguousarray(bow_match, np.int32)
        pts = np.ascontiguousarray(points, pkg.RELOC_POINT_DTYPE)
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        par = np.ascontiguousarray(params, pkg.RELOC_PNP_PARAMS_DTYPE).reshape(1)
        self.h = lib().amos_host_pnp_solver_create(_p(self.kps), len(self.kps), _p(bow), _p(pts), len(pts), _p(sig), len(sig), _p(par))
        if not self.h:
            raise RuntimeError(lib().amos_host_reloc_pnp_last_error().decode())

    def iterate(self, n_iterations):
        """-> (result record, inlier [n], generator state)."""
        result = np.zeros(1, self.pkg.RELOC_PNP_RESULT_DTYPE)
        inlier = np.zeros(max(len(self.kps), 1), np.uint8)
        rng = np.zeros(1, np.uint64)
        rc = lib().amos_host_pnp_solver_iterate(self.h, n_iterations, _p(result), _p(inlier), _p(rng))
        if rc != 0:
            raise RuntimeError(lib().amos_host_reloc_pnp_last_error().decode())
        return result[0], inlier[:len(self.kps)], int(rng[0])

    def close(self):
        if self.h:
            lib().amos_host_pnp_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def draw4(state, N):
    """-> (four indices, the generator state behind them) from amos_pnp_core.h's solver_draw4."""
    rng = np.array([state], np.uint64)
    idx = np.zeros(4, np.int32)
    lib().amos_host_pnp_draw4(_p(rng), N, _p(idx))
    return [int(i) for i in idx], int(rng[0])


def parameters(N, probability, min_inliers, max_iterations, epsilon):
    a, b, e = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32)
    lib().amos_host_pnp_parameters(N, probability, min_inliers, max_iterations, epsilon, _p(a), _p(b), _p(e))
    return int(a[0]), int(b[0]), np.float32(e[0])


def dropin(pkg, kps, K, level_sigma2, world, bad, vp_matches, seed, params, n_iterations, n_calls):
    """ORB_SLAM2::DevicePnPsolver on stand-ins -> list of dict(Tcw [16], has_pose, no_more, n_inliers, inliers [n]) per call, mean ms."""
    kps = np.ascontiguousarray(kps, pkg.KP_DTYPE)
    sig = np.ascontiguousarray(level_sigma2, np.float32)
    world = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
    bad = np.ascontiguousarray(bad, np.uint8)
    vp = np.ascontiguousarray(vp_matches, np.int32)
    n = len(kps)
    Tcw = np.zeros((n_calls, 16), np.float32)
    has_pose, no_more, n_inl = (np.zeros(n_calls, np.int32) for _ in range(3))
    inliers = np.zeros((n_calls, max(n, 1)), np.uint8)
    inl_flat = np.zeros(n_calls * max(n, 1), np.uint8)
    ms = C.c_double(0.0)
    rc = lib().amos_host_pnp_dropin(_p(kps), n, *[float(np.float32(x)) for x in K], _p(sig), len(sig), _p(world), _p(bad), len(world), _p(vp),
                                    C.c_uint64(seed), params["probability"], params["min_inliers"], params["max_iterations"], params["epsilon"],
                                    params["th2"], n_iterations, n_calls, _p(Tcw), _p(has_pose), _p(no_more), _p(n_inl), _p(inl_flat), C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"amos_host_pnp_dropin rc={rc}: {lib().amos_host_reloc_pnp_last_error().decode()}")
    inliers = inl_flat[:n_calls * n].reshape(n_calls, n) if n else inliers[:, :0]
    return [dict(Tcw=Tcw[c], has_pose=int(has_pose[c]), no_more=int(no_more[c]), n_inliers=int(n_inl[c]), inliers=inliers[c]) for c in range(n_calls)], ms.value
