"""CPU: the restatement of cv::solvePnPRansac(SOLVEPNP_P3P) + EPnP refit in tests/pnp_restatement.py (what amos_pnp_ransac_device is held to
bit for bit) checked against independent facts -- numpy.roots, numpy.linalg.eigh, the true pose of synthetic scenes, math.log -- and the C
entry points of amos_pnp_* validating their arguments before any device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

import pnp_restatement as pr

K = pr.K_TUM


def _real_roots(c):
    w = np.roots(c)
    return np.sort(w[np.abs(w.imag) < 1e-9 * np.maximum(1, np.abs(w))].real)


def test_quartic_roots_agree_with_numpy():
    rng = np.random.default_rng(31)
    for trial in range(300):
        kind = trial % 3
        if kind == 0:    # four real roots
            c = np.poly(np.sort(rng.uniform(-5, 5, 4))) * rng.uniform(0.5, 3)
        elif kind == 1:  # two real roots, one complex pair
            a, b = rng.uniform(-3, 3, 2)
            c = np.polymul(np.poly([a, a + rng.uniform(0.5, 3)]), [1.0, -2 * b, b * b + rng.uniform(0.5, 4)])
        else:            # all complex
            c = np.polymul([1.0, rng.uniform(-2, 2), rng.uniform(2, 5)], [1.0, rng.uniform(-2, 2), rng.uniform(2, 5)])
        got = pr.solve_quartic(*(float(v) for v in c))
        want = _real_roots(c)
        assert len(got) == len(want), (c, got, want)
        assert got == sorted(got)
        for g, w in zip(got, want):
            # 1e-12, widened where the roots cluster by the root's condition number: sum |c_k| |w|^k / |p'(w)| times a few eps
            cond = np.polyval(np.abs(c), abs(w)) / abs(np.polyval(np.polyder(c), w))
            assert abs(g - w) <= 1e-12 * max(1.0, abs(w)) + 64 * 2.2e-16 * cond, (c, got, want)
    # a double root: x^2 (x - 2)(x + 3) = x^4 + x^3 - 6 x^2 touches 0 from below at its local maximum x = 0.  The critical point is
    # bracketed to ~1e-47, where the computed value (-6 c^2) stays below 0: by the documented rule the tangent root is not counted;
    # the simple roots are exact
    assert pr.solve_quartic(1.0, 1.0, -6.0, 0.0, 0.0) == [-3.0, 2.0]
    # (x - 1)^2 (x^2 + 1): the double root is the only real one; every reported root lies within sqrt(eps) of it
    got = pr.solve_quartic(*np.polymul(np.poly([1.0, 1.0]), [1.0, 0.0, 1.0]))
    assert len(got) in (0, 1, 2) and all(abs(g - 1.0) < 1e-7 for g in got)
    assert pr.solve_quartic(1.0, 0.0, 0.0, 0.0, float("nan")) == []


@pytest.mark.parametrize("n", [3, 12])
def test_jacobi_matches_eigh(n):
    rng = np.random.default_rng(32 + n)
    for _ in range(20):
        A = rng.normal(0, 1, (n, n))
        A = A @ A.T if n == 12 else A + A.T
        lam, V = pr.jacobi_sym(A)
        order = pr.eig_order(lam, True)
        wl, wV = np.linalg.eigh(A)
        assert np.allclose(sorted(lam), wl, atol=1e-12 * np.abs(wl).max())
        for r, k in enumerate(order):
            w = wV[:, n - 1 - r]
            v = V[:, k]
            assert min(np.abs(v - w).max(), np.abs(v + w).max()) < 1e-9
            assert v[np.argmax(np.abs(v))] > 0
    # the 4 x 4 Jacobi of P3P's alignment
    A = rng.normal(0, 1, (4, 4))
    A = A + A.T
    D, U = pr.jacobi_4x4(list(A.reshape(16)))
    assert np.allclose(sorted(D), np.linalg.eigvalsh(A), atol=1e-12)
    U = np.array(U).reshape(4, 4)
    assert np.allclose(A @ U, U * np.array(D), atol=1e-12)


def _scene(seed, n, frac=0.0, noise=0.0, planar=False):
    return pr.scene(np.random.default_rng(seed), n, frac, noise, planar=planar)


def test_p3p_exact_correspondences():
    for seed in range(40):
        obj, img, Rt, _ = _scene(100 + seed, 4)
        sols, _, _ = pr.p3p_all(obj, img, *K)
        assert 1 <= len(sols) <= 4
        errs = [np.abs(np.array(s) - Rt).max() for s in sols]
        assert min(errs) < 2e-5, (seed, errs)   # float32 points: their rounding (~3e-5 px) bounds the pose error
        got = pr.p3p4(obj, img, *K)
        assert np.abs(np.array(got) - Rt).max() == min(errs)   # the 4th point picks the true one
    obj, img, _, _ = _scene(7, 4)
    obj[1] = obj[0]   # two identical 3-D points: no model
    assert pr.p3p4(obj, img, *K) is None


@pytest.mark.parametrize("n", [6, 50, 1000])
def test_epnp_exact_non_planar(n):
    obj, img, Rt, _ = _scene(200 + n, n)
    got = np.array(pr.epnp(obj, img, *K))
    # the points and projections are float32: the pose is exact up to their rounding (about 3e-5 px)
    assert np.abs(got - Rt).max() < (1e-6 if n == 6 else 2e-7), np.abs(got - Rt).max()
    R = got[:9].reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0


def test_epnp_planar_scene_is_finite():
    obj, img, Rt, _ = _scene(300, 500, planar=True)
    got = np.array(pr.epnp(obj, img, *K))
    assert np.isfinite(got).all()
    err = np.abs(got - Rt).max()
    # recorded: EPnP is poor on exactly planar sets (its null space has three extra directions once the third control point coincides
    # with the centroid); the result is a finite pose, and the RANSAC keeps its own model when the refit is not finite
    print(f"planar EPnP pose error {err:.3e}")
    R = got[:9].reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9


@pytest.mark.parametrize("frac", [0.0, 0.3, 0.5])
def test_ransac_recovers_the_true_pose(frac):
    obj, img, Rt, inl = _scene(400 + int(frac * 10), 1000, frac, 0.05)
    got, mask, st = pr.solve_pnp_ransac(obj, img, *K)
    assert st[0] == 1 and st[3] == 1000 and st[4] == 1 and st[1] == int(mask.sum())
    assert np.abs(got - Rt).max() < 2e-4, np.abs(got - Rt).max()
    m = mask.astype(bool)
    # the mask is the RANSAC mask (OpenCV's _inliers): no gross outlier in it, and the inliers of the minimal model it came from
    assert not (m & ~inl).any()
    assert (m & inl).sum() >= 0.99 * inl.sum()
    # the refit's pose explains every true inlier within the threshold
    e = pr.errors(got, obj, img, *K)
    assert (e[inl] <= np.float32(0.16)).all() and (e[~inl] > 1.0).all()


def test_ransac_small_and_special_inputs():
    obj, img, Rt, _ = _scene(500, 4)
    got, mask, st = pr.solve_pnp_ransac(obj, img, *K)
    assert st == (1, 4, 0, 4, 0) and mask.tolist() == [1, 1, 1, 1] and np.abs(got - Rt).max() < 2e-5
    assert pr.solve_pnp_ransac(obj[:3], img[:3], *K)[2] == (-1, 0, 0, 3, 0)
    obj, img, _, _ = _scene(501, 200, 0.6, 0.05)
    assert pr.solve_pnp_ransac(obj, img, *K, max_iters=5)[2][2] == 5


def test_iteration_count_matches_math_log():
    for ep in (0.1, 0.3, 0.5, 0.55):
        want = math.log(1 - 0.98) / math.log(1 - (1 - ep) ** 4)
        assert pr.update_num_iters(0.98, ep, 500) == min(500, int(round(want))), ep
    assert pr.update_num_iters(0.98, 0.0, 500) == 0 and pr.update_num_iters(0.98, 0.8, 500) == 500


def test_zero_rows_of_missing_depth_stay_in_the_list():
    """Tracking.cc:955-990 sizes the lists N and zero-fills them: a (0,0,0) -> (0,0) entry projects to (cx, cy) under any pose with
    t_z != 0... or to the principal point when R | t keeps it at depth t_z; it is an outlier of a pose that does not map the world origin
    onto the principal point, and it never breaks the sampler."""
    obj, img, Rt, inl = _scene(600, 400, 0.0, 0.05)
    obj[::5] = 0
    img[::5] = 0
    got, mask, st = pr.solve_pnp_ransac(obj, img, *K)
    assert st[0] == 1 and st[3] == 400
    assert not mask[::5].any()
    assert np.abs(got - Rt).max() < 2e-4


def test_pnp_entry_points_reject_bad_arguments(pkg):
    """amos_pnp_* validate before touching the device (this runs without a GPU)."""
    L = pkg.lib()
    h = C.c_void_p()
    assert L.amos_pnp_create(C.c_int(0), None, C.c_int(0), C.c_int(1), C.byref(h)) == -1 and not h.value
    assert L.amos_pnp_create(C.c_int(0), None, C.c_int(4097), C.c_int(1), C.byref(h)) == -1
    assert L.amos_pnp_create(C.c_int(0), None, C.c_int(100), C.c_int(0), C.byref(h)) == -1
    assert L.amos_pnp_create(C.c_int(0), None, C.c_int(100), C.c_int(1), None) == -1
    d = C.c_double
    buf = (C.c_float * 64)()
    Rt, st = (C.c_double * 12)(), (C.c_int32 * 5)()
    good = (d(535.4), d(539.2), d(320.1), d(247.6))
    assert L.amos_pnp_ransac_device(None, C.c_int(1), buf, buf, None, buf, None, *good, d(0.4), d(0.98), C.c_int(500), Rt, st, None) == -1
    assert L.amos_pnp_ransac(None, C.c_int(20), buf, buf, *good, d(0.4), d(0.98), C.c_int(500), Rt, None, st) == -1
    cam = pkg.SceneFlowCamera(320.1, 247.6, 1 / 535.4, 1 / 539.2)
    assert L.amos_pnp_scene_flow_device(None, buf, buf, buf, buf, buf, C.c_size_t(640), buf, C.c_size_t(640), C.c_int(640), C.c_int(480),
                                        C.byref(cam), d(535.4), d(539.2), Rt, st, None) == -1
    L.amos_pnp_stream.restype = C.c_void_p
    L.amos_pnp_stream.argtypes = [C.c_void_p]
    assert L.amos_pnp_stream(None) is None
    L.amos_pnp_destroy(None)
    assert len(L.amos_last_error()) > 0
