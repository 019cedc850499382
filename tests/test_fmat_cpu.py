"""CPU: the restatement of cv::findFundamentalMat(FM_RANSAC) in tests/fmat_restatement.py (what amos_fmat_ransac_device is held to bit for
bit) checked against independent facts -- numpy.roots, the epipolar constraint, the true F of synthetic two-view scenes -- and the C entry
points of amos_fmat_* validating their arguments before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import fmat_restatement as fr


def test_cubic_roots_agree_with_numpy():
    rng = np.random.default_rng(11)
    for trial in range(400):
        if trial % 2:
            r = np.sort(rng.uniform(-5, 5, 3))
            if trial % 4 == 1:  # a near-double root, the third one apart
                r0 = rng.uniform(-3, 3)
                r = np.array([r0, r0 + 10.0 ** -rng.uniform(1, 1.5), r0 + rng.choice([-1, 1]) * rng.uniform(2, 5)])
            c = np.poly(r) * rng.uniform(0.5, 3)
        else:
            c = rng.normal(0, 1, 4)
        n, got = fr.solve_cubic(tuple(float(v) for v in c))
        want = np.roots(c)
        real = np.sort(want[np.abs(want.imag) < 1e-9 * np.maximum(1, np.abs(want))].real)
        if n == 1 and len(real) == 3:   # three real roots closer than the discriminant resolves: accept one of them
            assert np.min(np.abs(real - got[0])) <= 1e-12 * max(1.0, abs(got[0])), (c, got, real)
            continue
        assert n == len(real), (c, n, real)
        for g, w in zip(sorted(got), real):
            assert abs(g - w) <= 1e-12 * max(1.0, abs(w)), (c, got, real)
    assert fr.solve_cubic((0.0, 0.0, 0.0, 0.0))[0] == -1 and fr.solve_cubic((0.0, 0.0, 0.0, 1.0))[0] == 0
    assert fr.solve_cubic((0.0, 0.0, 2.0, -1.0)) == (1, [0.5])
    n, r = fr.solve_cubic((0.0, 1.0, -3.0, 2.0))
    assert n == 2 and sorted(r) == [1.0, 2.0]


def test_log_and_iteration_count():
    rng = np.random.default_rng(12)
    for x in np.concatenate([10.0 ** rng.uniform(-300, 0, 200), rng.uniform(0.5, 1, 200)]):
        assert abs(fr.log_(float(x)) - np.log(x)) <= 4e-16 * max(1, abs(np.log(x)))
    # RANSACUpdateNumIters: log(1 - p) / log(1 - (1 - ep)^7), rounded; capped by the current count; 0 when every point is an inlier
    assert fr.update_num_iters(0.99, 0.3, 1000) == round(np.log(0.01) / np.log(1 - 0.7 ** 7))
    assert fr.update_num_iters(0.99, 0.6, 1000) == 1000 and fr.update_num_iters(0.99, 0.0, 1000) == 0
    assert fr.update_num_iters(0.99, 0.5, 200) == 200 and fr.round_even(2.5) == 2 and fr.round_even(3.5) == 4


def test_run7point_exact_correspondences():
    rng = np.random.default_rng(13)
    for trial in range(30):
        p1, p2, Ft, _ = fr.two_view(rng, 7)
        Fs = fr.run7point(p1, p2)
        assert 1 <= len(Fs) <= 3
        for F in Fs:
            M = np.array(F).reshape(3, 3)
            assert abs(np.linalg.det(M)) <= 1e-9 * np.abs(M).max() ** 3
            h1, h2 = np.c_[p1, np.ones(7)].astype(np.float64), np.c_[p2, np.ones(7)].astype(np.float64)
            res = np.abs(np.einsum("ij,jk,ik->i", h2, M, h1)) / np.abs(M).max()
            assert res.max() < 1e-6
        # the true F is one of the solutions
        assert min(np.abs(np.array(F) - Ft).max() / np.abs(Ft).max() for F in Fs) < 1e-4


@pytest.mark.parametrize("frac", [0.0, 0.3, 0.5])
def test_ransac_recovers_the_true_fundamental_matrix(frac):
    p1, p2, Ft, inl = fr.two_view(np.random.default_rng(14), 300, frac)
    F, mask, st = fr.find_fundamental_ransac(p1, p2)
    assert st[0] == 1 and st[1] == int(inl.sum()) and st[3] == 300 and 1 <= st[2] <= 1000
    assert F[8] == 1.0 and np.abs(F - Ft).max() <= 1e-6 * np.abs(Ft).max()
    assert np.array_equal(mask.astype(bool), inl)


def test_ransac_special_inputs():
    rng = np.random.default_rng(15)
    line = np.c_[rng.uniform(0, 640, 50), np.full(50, 240.0)].astype(np.float32)
    F, mask, st = fr.find_fundamental_ransac(line, line + np.float32(3))   # collinear: the sampler never passes
    assert st == (0, 0, 0, 50) and not F.any() and not mask.any()
    same = np.tile(np.float32([[100, 200]]), (40, 1))
    assert fr.find_fundamental_ransac(same, same)[2] == (0, 0, 0, 40)
    p1, p2, _, _ = fr.two_view(rng, 10)
    assert fr.find_fundamental_ransac(p1, p2)[2] == (-1, 0, 0, 10)
    assert fr.find_fundamental_ransac(p1[:3], p2[:3])[2] == (0, 0, 0, 3)
    p1, p2, _, _ = fr.two_view(rng, 100, 0.6)
    assert fr.find_fundamental_ransac(p1, p2, max_iters=5)[2][2] == 5


def test_error_keeps_a_nan_first_term():
    """std::max(e1, e2) = e1 < e2 ? e2 : e1: with F = [[0, 0, 1], [0, 0, 0], [0, 0, 0]] and x2 = 0, e2 = 0 and e1 = 0 * inf = NaN; the
    error is NaN and the point is not an inlier (flow_oracle.fundamental_errors, the scorer kernel's check, follows the same rule)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import flow_oracle as fo
    F = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 0]], np.float64)
    p1, p2 = np.array([[5, 7], [5, 7]], np.float32), np.array([[0, 2], [3, 2]], np.float32)
    for e in (fr.errors(F, p1, p2), fo.fundamental_errors(F, p1, p2)):
        assert e.dtype == np.float32 and np.isnan(e[0]) and np.isinf(e[1])
        assert not (e <= np.float32(0.1 * 0.1)).any()


def test_rng_is_opencvs_multiply_with_carry():
    r = fr.Rng()
    a = [r.next() for _ in range(3)]
    s = (1 << 64) - 1
    for v in a:
        s = ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32)) % (1 << 64)
        assert v == s & 0xFFFFFFFF
    assert a[0] == (0xFFFFFFFF * 4164903690 + 0xFFFFFFFF) & 0xFFFFFFFF


def test_fmat_entry_points_reject_bad_arguments(pkg):
    """amos_fmat_* validate before touching the device (this runs without a GPU)."""
    L = pkg.lib()
    h = C.c_void_p()
    assert L.amos_fmat_create(C.c_int(0), None, C.c_int(0), C.c_int(1), C.byref(h)) == -1 and not h.value
    assert L.amos_fmat_create(C.c_int(0), None, C.c_int(4097), C.c_int(1), C.byref(h)) == -1
    assert L.amos_fmat_create(C.c_int(0), None, C.c_int(100), C.c_int(0), C.byref(h)) == -1
    assert L.amos_fmat_create(C.c_int(0), None, C.c_int(100), C.c_int(1), None) == -1
    d = C.c_double
    buf = (C.c_float * 64)()
    F, st = (C.c_double * 9)(), (C.c_int32 * 4)()
    assert L.amos_fmat_ransac_device(None, C.c_int(1), buf, buf, None, buf, None, d(0.1), d(0.99), C.c_int(1000), F, st, None) == -1
    assert L.amos_fmat_ransac(None, C.c_int(20), buf, buf, d(0.1), d(0.99), C.c_int(1000), F, None, st) == -1
    assert L.amos_fmat_scene_flow_pair_device(None, buf, buf, buf, buf, F, F, buf, st) == -1
    L.amos_fmat_stream.restype = C.c_void_p
    L.amos_fmat_stream.argtypes = [C.c_void_p]
    assert L.amos_fmat_stream(None) is None
    L.amos_fmat_destroy(None)
    assert len(L.amos_last_error()) > 0
