"""ctypes binding of tests/host_bow/libamos_host_bow_test.so: ORB_SLAM2::DeviceVocabulary (text loader, transform through ComputeBoW) and
SearchByBoW(pKF, F, ...) on stand-in Frame / KeyFrame / MapPoint objects, through the drop-in of amos-slam_amd/host/FrameBoW.h ("dropin") or
through the host class ORBmatcherFor::SearchByBoW ("parent")."""
import ctypes as C
import os

import numpy as np

import bow_search_cases as bc
import host_binding as hb

SO = os.path.join(hb.ROOT, "tests", "host_bow", "libamos_host_bow_test.so")

_lib = None


def lib():
    global _lib
    if _lib is None:
        hb.host()  # the HIP runtime and the product libraries first
        _lib = C.CDLL(SO)
        _lib.amos_host_bow_last_error.restype = C.c_char_p
        _lib.amos_host_bow_voc_load.restype = C.c_void_p
        _lib.amos_host_bow_voc_load.argtypes = [C.c_char_p, C.c_void_p]
        _lib.amos_host_bow_voc_free.argtypes = [C.c_void_p]
        _lib.amos_host_bow_voc_arrays.argtypes = [C.c_void_p] * 6
        _lib.amos_host_compute_bow.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
        _lib.amos_host_bow_search.argtypes = ([C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
                                              + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
                                              + [C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
    return _lib


def last_error():
    return lib().amos_host_bow_last_error().decode()


class Vocabulary:
    """DeviceVocabulary::loadFromTextFile(path); .status is AMOS_OK (0) or AMOS_ERR_INVALID (-1), .error the loader's text"""

    def __init__(self, path):
        status = C.c_int32(0)
        self.h = lib().amos_host_bow_voc_load(str(path).encode(), C.byref(status))
        self.status, self.error = status.value, last_error()

    def arrays(self):
        """-> dict(k, L, scoring, weighting, nodes, words, parent, is_leaf, desc, weight)"""
        info = np.zeros(6, np.int32)
        lib().amos_host_bow_voc_arrays(self.h, hb._p(info), None, None, None, None)
        n = int(info[4])
        parent, leaf, desc, weight = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.float64)
        lib().amos_host_bow_voc_arrays(self.h, hb._p(info), hb._p(parent), hb._p(leaf), hb._p(desc), hb._p(weight))
        return dict(zip(("k", "L", "scoring", "weighting", "nodes", "words"), map(int, info)), parent=parent, is_leaf=leaf, desc=desc, weight=weight)

    def compute_bow(self, desc, levelsup=4, prefilled=False):
        """ORB_SLAM2::ComputeBoW on a stand-in frame -> dict(words, word_weights, node_ids, node_off, node_idx): mBowVec and mFeatVec flattened"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        counts, words, wts = np.zeros(3, np.int32), np.zeros(m, np.uint32), np.zeros(m, np.float64)
        ids, off, idx = np.zeros(m, np.uint32), np.zeros(m + 1, np.int32), np.zeros(m, np.int32)
        rc = lib().amos_host_compute_bow(self.h, n, hb._p(desc), levelsup, int(prefilled), hb._p(counts), hb._p(words), hb._p(wts), hb._p(ids),
                                         hb._p(off), hb._p(idx))
        if rc != 0:
            raise RuntimeError(f"amos_host_compute_bow rc={rc}: {last_error()}")
        w, a, j = map(int, counts)
        return dict(words=words[:w], word_weights=wts[:w], node_ids=ids[:a], node_off=off[:a + 1], node_idx=idx[:j])

    def close(self):
        if self.h:
            lib().amos_host_bow_voc_free(self.h)
            self.h = None

    __del__ = close


def search_by_bow(which, kf, f, nn_ratio, check_orientation, bad_points=None, repeat=1):
    """kf, f: sides of bow_search_cases; bad_points: keyframe features whose map point isBad().  -> dict(n_matches, match, ms)"""
    kid, koff, kidx = bc.csr(kf["fv"])
    fid, foff, fidx = bc.csr(f["fv"])
    n_kf, n_f = len(kf["desc"]), len(f["desc"])
    point = np.ones(n_kf, np.uint8) if kf.get("has_point") is None else np.ascontiguousarray(kf["has_point"], np.uint8).copy()
    if bad_points is not None:
        point[np.asarray(bad_points, int)] = 2
    kk, fk = np.ascontiguousarray(kf["keys"], hb.KP), np.ascontiguousarray(f["keys"], hb.KP)
    kd, fd = np.ascontiguousarray(kf["desc"], np.uint8), np.ascontiguousarray(f["desc"], np.uint8)
    match, ms = np.zeros(max(n_f, 1), np.int32), C.c_double(0)
    n = lib().amos_host_bow_search(n_kf, hb._p(kk), hb._p(kd), hb._p(point), len(kid), hb._p(kid), hb._p(koff), hb._p(kidx), n_f, hb._p(fk), hb._p(fd),
                                   len(fid), hb._p(fid), hb._p(foff), hb._p(fidx), float(nn_ratio), int(check_orientation),
                                   {"dropin": 0, "parent": 1}[which], repeat, hb._p(match), C.byref(ms))
    if n < 0:
        raise RuntimeError(f"amos_host_bow_search rc={n}: {last_error()}")
    return dict(n_matches=n, match=match[:n_f], ms=ms.value)
