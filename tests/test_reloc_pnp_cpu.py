"""Relocalization's PnPsolver without a GPU: the restatement (tests/reloc_pnp_restatement.py) on its own -- the iteration-count table, the
draw, CheckInliers, noise-free and outlier-ridden scenes -- then the host compilation of amos_pnp_core.h's solver pieces
(tests/host_reloc_pnp) against it bit for bit on every shape of the GPU tests, and the new entry points of the library with every argument
they refuse."""
import ctypes as C
import math

import numpy as np
import pytest

import host_reloc_pnp_binding as hp
import pnp_restatement as pr
import reloc_pnp_cases as rc
import reloc_pnp_restatement as rp
from fmat_restatement import Rng

f32 = np.float32


def test_iteration_count_table_against_math_log():
    """SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991): nMin = max(int(N * 0.5), 10), eps = max(0.5, nMin / N) in float, and
    ceil(log(0.01) / log(1 - eps^3)) -- the quotient is never closer than 0.105 to an integer for N = 10 .. 4096, so the restated log and
    libm's agree on the ceiling."""
    table = {10: 1, 11: 4, 12: 6, 13: 8, 14: 11, 15: 14, 16: 17, 17: 21, 18: 25, 19: 30}
    closest = 1.0
    for N in range(10, 4097):
        n_min, its, eps = rp.ransac_parameters(N, 0.99, 10, 300, 0.5)
        assert n_min == max(N // 2, 10)
        e = float(f32(max(f32(0.5), f32(n_min) / f32(N))))
        assert float(eps) == e
        if n_min == N:
            want = 1
        else:
            q = math.log(1 - 0.99) / math.log(1 - e ** 3)
            closest = min(closest, abs(q - round(q)))
            want = max(1, min(int(math.ceil(q)), 300))
        assert its == want == table.get(N, 35), N
        assert hp.parameters(N, 0.99, 10, 300, 0.5) == (n_min, its, eps), N
    print("closest quotient to an integer:", closest)
    assert closest > 0.1


def test_parameters_at_the_edges():
    assert rp.ransac_parameters(0, 0.99, 10, 300, 0.5) == (10, 35, f32(0.5)) == hp.parameters(0, 0.99, 10, 300, 0.5)  # N = 0: eps is not raised
    assert rp.ransac_parameters(3, 0.99, 10, 300, 0.5)[:2] == (10, 1)  # eps = 10 / 3: 1 - eps^3 < 0
    assert rp.ransac_parameters(100, 0.99, 1, 300, 0.01)[0] == 4       # raised to the minimal set
    assert rp.ransac_parameters(100, 0.99, 10, 7, 0.5)[1] == 7         # min(nIterations, maxIts)
    for N, p, mi, mx, e in ((3, 0.99, 10, 300, 0.5), (100, 0.99, 1, 300, 0.01), (100, 0.99, 10, 7, 0.5), (4096, 0.5, 8, 300, 0.4), (50, 0.999999, 8, 65536, 0.2)):
        assert hp.parameters(N, p, mi, mx, e) == rp.ransac_parameters(N, p, mi, mx, e), (N, p, mi, mx, e)


def literal_draw4(rng, N):
    """PnPsolver.cc:268-283 with the copied index list."""
    avail = list(range(N))
    out = []
    for _ in range(4):
        randi = rp.random_int(rng, len(avail))
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


@pytest.mark.parametrize("N", [4, 5, 7, 10, 64, 4096])
def test_draw_equals_the_literal_swap_with_back(N):
    a, b = Rng(12345 + N), Rng(12345 + N)
    state = 12345 + N
    for _ in range(300):
        got, want = rp.draw4(a, N), literal_draw4(b, N)
        assert got == want and len(set(got)) == 4 and all(0 <= i < N for i in got)
        host, state = hp.draw4(state, N)
        assert host == want and state == a.s == b.s


def test_draw_from_one_entry_gives_index_0():
    r = Rng(99)
    for _ in range(1000):
        assert rp.random_int(r, 1) == 0


def loop_check_inliers(Rt, P3D, P2D, max_err, fu, fv, uc, vc):
    """CheckInliers written as the reference's loop, one correspondence at a time."""
    out = []
    with np.errstate(all="ignore"):
        for i in range(len(P3D)):
            X, Y, Z = (np.float64(P3D[i][k]) for k in range(3))
            Xc = f32(((Rt[0] * X + Rt[1] * Y) + Rt[2] * Z) + Rt[9])
            Yc = f32(((Rt[3] * X + Rt[4] * Y) + Rt[5] * Z) + Rt[10])
            invZc = f32(np.float64(1.0) / (((Rt[6] * X + Rt[7] * Y) + Rt[8] * Z) + Rt[11]))
            ue = uc + (fu * np.float64(Xc)) * np.float64(invZc)
            ve = vc + (fv * np.float64(Yc)) * np.float64(invZc)
            dx, dy = f32(np.float64(P2D[i][0]) - ue), f32(np.float64(P2D[i][1]) - ve)
            out.append(bool(dx * dx + dy * dy < max_err[i]))
    return np.array(out, bool)


def test_check_inliers_against_the_loop_form():
    rng = np.random.default_rng(5)
    obj, img, Rt, inl = pr.scene(rng, 60, 0.3, 0.5)
    Rt = [np.float64(x) for x in Rt]
    max_err = (rng.choice(rc.LEVEL_SIGMA2[:3], 60) * f32(5.991)).astype(f32)
    got = rp.check_inliers(Rt, obj, img, max_err, *pr.K_TUM)
    assert np.array_equal(got, loop_check_inliers(Rt, obj, img, max_err, *pr.K_TUM))
    assert got[inl].mean() > 0.9 and not got[~inl].any()
    bad = list(Rt)
    bad[11] = np.float64(np.nan)
    assert not rp.check_inliers(bad, obj, img, max_err, *pr.K_TUM).any()  # a NaN fails the test
    assert not loop_check_inliers(bad, obj, img, max_err, *pr.K_TUM).any()


def dense_pair(obj, img, octave=0):
    """Every feature a correspondence: feature i names point i."""
    n = len(obj)
    kps = np.zeros(n, rc.KP)
    kps["x"], kps["y"], kps["octave"] = img[:, 0], img[:, 1], octave
    points = np.zeros(n, rc.POINT)
    points["pos"] = obj
    return dict(kps=kps, bow_match=np.arange(n, dtype=np.int32), points=points, K=pr.K_TUM)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_free_scene_returns_a_refined_pose_at_once(seed):
    obj, img, Rt, _ = pr.scene(np.random.default_rng(seed), 40)
    pair = dense_pair(obj, img)
    (r, _), = rc.run_restatement(pair, seed, n_calls=1)
    assert r.has_pose and r.refined and not r.no_more and r.n_correspondences == 40 and (r.min_inliers, r.max_iterations) == (20, 35)
    max_err = np.full(40, rc.LEVEL_SIGMA2[0] * f32(5.991), f32)
    T = r.Tcw.astype(np.float64)
    Rt32 = [T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10], T[3], T[7], T[11]]
    assert rp.check_inliers(Rt32, obj, img, max_err, *pr.K_TUM).all()  # error2 < sigma2 * 5.991 for every correspondence
    assert r.n_inliers == 40 and r.inlier.all()
    assert np.abs(np.array(Rt32) - Rt).max() < 1e-3


def test_seventy_percent_outliers_run_out_of_iterations():
    """N = 40 with 28 outliers: minInliers = 20 is out of reach of a 12-inlier scene, so the first call runs max(maxIts, 5) = 35
    iterations, sets bNoMore and returns no pose.  Recorded for seed 7: iterations 35, best_inliers 0, no pose."""
    obj, img, _, _ = pr.scene(np.random.default_rng(7), 40, 0.7, 0.5)
    (r, _), = rc.run_restatement(dense_pair(obj, img), 7, n_calls=1)
    print("out70:", r.iterations, r.has_pose, r.n_inliers, r.best_inliers)
    assert r.iterations == r.iterations_call == 35 and r.no_more
    assert (r.has_pose and not r.refined and r.n_inliers >= 20) or (not r.has_pose and r.n_inliers == 0 and not r.inlier.any())
    assert (r.has_pose, r.best_inliers) == (0, 0)


def params_of(pkg, pair, seed, **kw):
    return pkg.reloc_pnp_params([f32(x) for x in pair["K"]], seed, n_iterations=rc.N_ITERATIONS, **dict(rc.REFERENCE, **kw))


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_host_compiled_solver_equals_the_restatement(pkg, name):
    pair, seed, want = rc.case(name)
    s = hp.HostSolver(pkg, pair["kps"], pair["bow_match"], pair["points"], rc.LEVEL_SIGMA2, params_of(pkg, pair, seed))
    for call, (w, rng) in enumerate(want):
        got, inlier, state = s.iterate(rc.N_ITERATIONS)
        print(name, call, {f: int(got[f]) for f in rc.RESULT_FIELDS})
        rc.assert_result_equal(got, inlier, w, f"{name} call {call}")
        assert state == rng, f"{name} call {call}: generator state"
    s.close()
    assert want[0][0].n_correspondences == rc.CASES[name][0]


def test_cases_cover_both_ends_of_the_first_call():
    """The carried-state calls are checked behind a first call that returned through Refine and behind one that set bNoMore."""
    first = {name: rc.case(name)[2][0][0] for name in rc.CASES}
    assert any(r.refined and not r.no_more for r in first.values()) and any(r.no_more and r.iterations > 0 for r in first.values())
    assert first["n9"].no_more and first["n9"].iterations == 0 and first["n10"].max_iterations == 1
    fails = rc.case("refine_fails")[2]
    assert all(r.has_pose and r.no_more and not r.refined and r.n_solves > r.iterations for r, _ in fails)  # Refine ran and failed
    assert fails[2][0].n_solves - fails[0][0].n_solves > 10  # and again in a later call on the same best set
    degenerate = rc.case("duplicates_outliers")[2][-1][0]
    assert degenerate.n_nonfinite > 0 and degenerate.iterations >= 21  # minimal solves with a pose that is not finite count zero inliers
    later = [rc.case(name)[2][2][0] for name in rc.CASES]
    assert any(r.has_pose for r in later)


def test_octave_outside_the_table_and_match_outside_the_points_set_status():
    pair, seed, _ = rc.case("n20")
    pair = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pair.items()}
    feats = np.nonzero(pair["bow_match"] >= 0)[0]
    pair["kps"]["octave"][feats[0]] = len(rc.LEVEL_SIGMA2)
    pair["kps"]["octave"][feats[1]] = -1
    pair["bow_match"][feats[2]] = len(pair["points"])
    (r, _), = rc.run_restatement(pair, seed, n_calls=1)
    assert r.status == 3 and 16 <= r.n_correspondences <= 18


def test_too_many_correspondences_give_code_minus_3(pkg):
    n = rp.MAX_CORRESPONDENCES + 1
    rng = np.random.default_rng(3)
    obj, img, _, _ = pr.scene(rng, n)
    pair = dense_pair(obj, img)
    (r, _), = rc.run_restatement(pair, 1, n_calls=1)
    assert r.code == -3 and r.n_correspondences == n and not r.has_pose
    s = hp.HostSolver(pkg, pair["kps"], pair["bow_match"], pair["points"], rc.LEVEL_SIGMA2, params_of(pkg, pair, 1))
    got, inlier, _ = s.iterate(5)
    assert int(got["code"]) == -3 and int(got["n_correspondences"]) == n and not inlier.any()


def test_library_exports_the_reloc_pnp_entry_points(pkg):
    names = ("amos_match_reloc_pnp_batch_device", "amos_match_reloc_pnp", "amos_reloc_pnp_state_bytes")
    L = C.CDLL(pkg.LIB_PATH)
    for name in names:
        assert name in pkg.EXPORTS and hasattr(L, name), name
    assert hasattr(pkg.OrbMatcher, "reloc_pnp_batch_device") and hasattr(pkg.OrbMatcher, "reloc_pnp")
    assert (pkg.RELOC_PNP_PARAMS_DTYPE.itemsize, pkg.RELOC_PNP_RESULT_DTYPE.itemsize) == (64, 104)
    assert (C.sizeof(pkg.RelocPnpParams), C.sizeof(pkg.RelocPnpResult), C.sizeof(pkg.RelocPnp)) == (64, 104, 13 * 8 + 16)
    for f in rc.RESULT_FIELDS + ("Tcw", "skipped"):
        assert f in pkg.RELOC_PNP_RESULT_DTYPE.names
    assert pkg.RELOC_POINT_DTYPE == rc.POINT and pkg.KP_DTYPE == rc.KP
    small, large = pkg.reloc_pnp_state_bytes(1), pkg.reloc_pnp_state_bytes(65536)
    assert small % 64 == 0 and large == pkg.reloc_pnp_state_bytes(4096) and large - pkg.reloc_pnp_state_bytes(2048) == 2048 * 48


def test_invalid_arguments_return_before_the_device_is_touched(pkg):
    """No GPU here: every refusal comes back as AMOS_ERR_INVALID (-1) with the entry's name in the message; the handle is a dummy that is
    read only after the checks have passed, and every device pointer is NULL or points at host memory that nothing may touch."""
    L = pkg.lib()
    fake = C.create_string_buffer(1024)
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    K = (500.0, 500.0, 320.0, 240.0)
    base = dict(d_kps=p, d_counts=p, d_points=p, d_bow_match=p, d_state=p, d_result=p, d_inlier=p, d_match=p, d_found=None, n_frames=2, capacity=100,
                fop=[0, 1, 0], off=[0, 10, 10, 30], sig=rc.LEVEL_SIGMA2, par=[dict() for _ in range(3)])

    def call(handle=fake, **kw):
        a = dict(base, **kw)
        fop, off = np.asarray(a["fop"], np.int32), np.asarray(a["off"], np.int32)
        par = np.array([pkg.reloc_pnp_params(K, 1, **d) for d in a["par"]], pkg.RELOC_PNP_PARAMS_DTYPE)
        s = pkg.RelocPnp(a["d_kps"], a["d_counts"], None if a.get("no_fop") else fop.ctypes.data, None if a.get("no_off") else off.ctypes.data,
                         a["d_points"], a["d_bow_match"], None if a.get("no_sig") else a["sig"].ctypes.data,
                         None if a.get("no_par") else par.ctypes.data, a["d_state"], a["d_result"], a["d_inlier"], a["d_match"], a["d_found"],
                         a["n_frames"], a.get("n_pairs", len(par)), a["capacity"], a.get("n_levels", len(a["sig"])))
        rcode = L.amos_match_reloc_pnp_batch_device(handle, C.byref(s))
        if rcode == -1:
            assert b"amos_match_reloc_pnp_batch_device" in L.amos_last_error()
        return rcode
    assert call(handle=None) == -1 and L.amos_match_reloc_pnp_batch_device(fake, None) == -1
    for name in ("d_kps", "d_counts", "d_points", "d_bow_match", "d_state", "d_result", "d_inlier", "d_match"):
        assert call(**{name: None}) == -1, name
    for name in ("no_fop", "no_off", "no_sig", "no_par"):
        assert call(**{name: True}) == -1, name
    assert call(n_pairs=0) == -1 and call(n_frames=0) == -1
    assert call(capacity=0) == -1 and call(capacity=65537) == -1
    assert call(n_levels=0) == -1 and call(n_levels=1000) == -1
    assert call(fop=[0, 2, 0]) == -1 and call(fop=[0, -1, 0]) == -1
    assert call(off=[0, 10, 9, 30]) == -1 and call(off=[-1, 10, 10, 30]) == -1
    bads = (dict(probability=0.0), dict(probability=1.0), dict(probability=np.nan), dict(epsilon=0.0), dict(epsilon=-0.5), dict(epsilon=np.inf),
            dict(epsilon=np.nan), dict(th2=0.0), dict(th2=np.nan), dict(th2=np.inf), dict(max_iterations=0), dict(n_iterations=0),
            dict(max_iterations=65537), dict(n_iterations=65537))
    for bad in bads:
        assert call(par=[dict(), bad, dict()]) == -1, bad
    # the host form
    kp, bow, pts = np.zeros(4, pkg.KP_DTYPE), np.full(4, -1, np.int32), np.zeros(2, pkg.RELOC_POINT_DTYPE)
    state = np.zeros(pkg.reloc_pnp_state_bytes(4), np.uint8)
    res, inl, mt, fd = np.zeros(1, pkg.RELOC_PNP_RESULT_DTYPE), np.zeros(4, np.uint8), np.zeros(4, np.int32), np.zeros(2, np.uint8)

    def host(handle=fake, kps=kp, n=4, bow_=bow, points=pts, n_points=2, sig=rc.LEVEL_SIGMA2, n_levels=8, par=dict(), state_=state, result=res,
             inlier=inl, match=mt, found=fd):
        par = None if par is None else np.array([pkg.reloc_pnp_params(K, 1, **par)], pkg.RELOC_PNP_PARAMS_DTYPE)
        rcode = L.amos_match_reloc_pnp(handle, pkg._p(kps), n, pkg._p(bow_), pkg._p(points), n_points, pkg._p(sig), n_levels, pkg._p(par),
                                       pkg._p(state_), pkg._p(result), pkg._p(inlier), pkg._p(match), pkg._p(found))
        if rcode == -1:
            assert b"amos_match_reloc_pnp:" in L.amos_last_error()
        return rcode
    assert host(handle=None) == -1 and host(par=None) == -1 and host(sig=None) == -1 and host(state_=None) == -1 and host(result=None) == -1
    assert host(n=-1) == -1 and host(n=65537) == -1 and host(n_points=-1) == -1 and host(n_levels=0) == -1
    assert host(kps=None) == -1 and host(bow_=None) == -1 and host(inlier=None) == -1 and host(match=None) == -1
    assert host(points=None) == -1 and host(found=None) == -1
    for bad in bads:
        assert host(par=bad) == -1, bad
