"""Optimizer::PoseOptimization without a GPU: the pieces of amos-slam_amd/csrc/amos_pose_core.h as tests/pose_optimization_restatement.py
restates them (sin_cos, the LDL^T solve, the fixed-order sum), the restatement against the independent g2o-form, the recovery of a known
pose, the header compiled as a plain C++ program against the restatement bit for bit, and the C entries' argument checks."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pose_optimization_cases as pc
import pose_optimization_g2o_form as gf
import pose_optimization_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "amos-slam_amd", "csrc", "amos_pose_core.h")
EPS = 2.0 ** -52
# The largest |Rt(restatement) - Rt(g2o-form)| over pc.all_cases(), measured: the two differ by the order of the sums
# (and sin / cos, the cube, the solve) amplified by the system's condition.  The test allows 16 times that: room for another seed.
MEASURED_DELTA_RT = 9.2e-11


def header_constant(name):
    text = open(HEADER).read()
    return float(re.search(rf"constexpr double {name} = ([0-9.eE+-]+);", text).group(1))


def test_sin_cos_on_the_grid_and_at_large_arguments():
    bound = header_constant("kSinCosUlp") + 1.0  # the header's measured worst error plus one ulp
    worst_s = worst_c = 0.0
    for x in np.linspace(1e-5, 2.0 * math.pi, 200001):
        s, c = pr.sin_cos(float(x))
        rs, rc = math.sin(x), math.cos(x)
        worst_s, worst_c = max(worst_s, abs(s - rs) / math.ulp(rs)), max(worst_c, abs(c - rc) / math.ulp(rc))
    print(f"sin_cos on [1e-5, 2 pi]: worst {worst_s} ulp (sin), {worst_c} ulp (cos)")
    assert worst_s <= bound and worst_c <= bound
    rng = np.random.default_rng(0)
    for x in rng.uniform(2.0 * math.pi, pr.REDUCE_BIG, 2000):  # the exact reduction: an absolute error of a rounding or two
        s, c = pr.sin_cos(float(x))
        assert abs(s - math.sin(x)) <= 2 * EPS and abs(c - math.cos(x)) <= 2 * EPS, x
    for x in (65536.0, 1e5, 1e6, 123456789.0, 1e10, 1e13):  # theta mod fl(2 pi): off by (theta / 2 pi) (2 pi - fl(2 pi)) in the argument
        s, c = pr.sin_cos(x)
        off = x / (2.0 * math.pi) * 2.4492935982947064e-16 + 2 * EPS
        assert abs(s - math.sin(x)) <= off and abs(c - math.cos(x)) <= off, x
    for x in (1e22, 1e300, 1.7976931348623157e308, 2.0 ** 52 + 1.0):  # defined for every finite theta: a sine and cosine of SOME angle
        s, c = pr.sin_cos(x)
        assert abs(s * s + c * c - 1.0) <= 8 * EPS, x


def test_ldlt_against_numpy():
    rng = np.random.default_rng(1)

    def upper(A):
        return [float(A[i, j]) for i in range(6) for j in range(i, 6)]
    for trial in range(200):
        M = rng.normal(size=(8, 6)) * rng.uniform(0.1, 100.0, 6)
        A = M.T @ M
        lam = float(rng.uniform(0, 1e-3) * np.abs(np.diag(A)).max())
        b = rng.normal(size=6)
        ok, x = pr.solve6(upper(A), lam, [float(v) for v in b], [0.0] * 6)
        ref = np.linalg.solve(A + lam * np.eye(6), b)
        assert ok, trial
        assert np.linalg.norm(np.array(x) - ref) <= 64 * np.linalg.cond(A + lam * np.eye(6)) * EPS * np.linalg.norm(ref), trial
    for trial in range(50):  # indefinite: some pivot of D is negative (Sylvester), the solve fails and x is left alone
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        d = rng.uniform(0.5, 10.0, 6) * np.where(np.arange(6) == trial % 6, -1.0, 1.0)
        A = Q @ np.diag(d) @ Q.T
        A = (A + A.T) / 2
        keep = [float(v) for v in rng.normal(size=6)]
        ok, x = pr.solve6(upper(A), 0.0, [1.0] * 6, keep)
        assert not ok and x == keep, trial
    for trial in range(20):  # singular with exact zero pivots: those components are zero, the rest solves the block
        M = rng.normal(size=(7, 4))
        A = np.zeros((6, 6))
        idx = rng.permutation(6)[:4]
        A[np.ix_(idx, idx)] = M.T @ M
        b = rng.normal(size=6)
        ok, x = pr.solve6(upper(A), 0.0, [float(v) for v in b], [0.0] * 6)
        ref = np.linalg.solve(M.T @ M, b[idx])
        rest = [i for i in range(6) if i not in idx]
        assert ok and all(x[i] == 0.0 for i in rest), trial
        assert np.linalg.norm(np.array(x)[idx] - ref) <= 64 * np.linalg.cond(M.T @ M) * EPS * np.linalg.norm(ref), trial


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 300, 1000, 5000])
def test_fixed_order_sum_against_fsum(n):
    rng = np.random.default_rng(n)
    terms = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)
    active = rng.random(n) < 0.8
    got = pr.tree_sum(pr.strided_partials(terms, active))
    assert abs(got - math.fsum(terms[active])) <= n * EPS * float(np.abs(terms[active]).sum())
    sub = pr.tree_sum(pr.strided_partials(terms, active, subtract=True))
    assert sub == -got  # subtraction from 0.0 mirrors the additions exactly
    explicit = [0.0] * pr.K_THREADS  # the order spelled out: partial t adds edges t, t + 256, ...; blocks of 64 fold; (B0 + B1) + (B2 + B3)
    for e in range(n):
        if active[e]:
            explicit[e % pr.K_THREADS] += float(terms[e])
    for blk in range(0, pr.K_THREADS, 64):
        s = 32
        while s:
            for i in range(s):
                explicit[blk + i] += explicit[blk + i + s]
            s >>= 1
    assert got == (explicit[0] + explicit[64]) + (explicit[128] + explicit[192])


@pytest.fixture(scope="module")
def cases():
    return pc.all_cases()


@pytest.fixture(scope="module")
def both(cases):
    """{name: (restatement result, flags per edge, g2o-form dict)}, computed once"""
    out = {}
    for name, c in cases.items():
        g = gf.pose_optimization(c)
        res, flags = pr.optimize_edges(g["edges"], c["camera"])
        out[name] = (res, flags, g)
    return out


def test_restatement_against_the_g2o_form(cases, both):
    left_out, worst = [], 0.0
    for name, (res, flags, g) in both.items():
        E = g["edges"]
        if g["chi2"] is not None:
            thr = np.where(E.stereo, 7.815, 5.991)
            if (np.abs(g["chi2"] - thr) <= 1e-6 * thr).any():  # an edge on the threshold may fall either way
                left_out.append(name)
                continue
        assert (flags is None) == (g["outlier"] is None), name
        assert flags is None or np.array_equal(flags, g["outlier"]), name
        assert int(res["n_inliers"]) == g["ret"], name
        d = np.abs(np.asarray(res["Rt"]) - g["Rt"])
        assert np.isfinite(d).all(), name
        worst = max(worst, float(d.max()))
        assert d.max() <= 16 * MEASURED_DELTA_RT, (name, d.max())
        a, b = np.asarray(res["Rt"]).astype(np.float32), g["Rt"].astype(np.float32)
        for i in np.nonzero(a != b)[0]:  # one float ulp apart, and only across a rounding boundary
            lo, hi = min(a[i], b[i]), max(a[i], b[i])
            assert np.nextafter(lo, np.float32(np.inf)) == hi, (name, i)
            boundary = (float(lo) + float(hi)) / 2.0
            assert abs(res["Rt"][i] - boundary) <= MEASURED_DELTA_RT and abs(g["Rt"][i] - boundary) <= MEASURED_DELTA_RT, (name, i)
    print(f"largest |Rt(restatement) - Rt(g2o-form)| over {len(both)} cases: {worst}")
    assert left_out == []


def test_the_odd_branches_are_reached(both):
    by = {k: v[0] for k, v in both.items()}
    assert by["2_mono_0"]["rounds"] == 0 and by["2_mono_0"]["n_inliers"] == 0 and by["3_mono_0"]["rounds"] == 1 and by["9_stereo_25"]["rounds"] == 1
    assert by["10_mono_0"]["rounds"] == 4 and by["count_zero"]["n_edges"] == 0
    assert tuple(by["exact_optimum"]["iterations"]) == (1, 1, 1, 1) and tuple(by["exact_optimum"]["chi2"]) == (0.0,) * 4   # rho == 0
    assert not np.isfinite(by["zero_depth_mono"]["chi2"][0]) and not np.isfinite(by["zero_depth_stereo"]["chi2"][0])      # the NaN path
    assert by["bad_octave"]["n_edges"] == 48 and by["bad_match_index"]["n_edges"] == 49
    neg = pc.restate(pc.negative_sigma_case())[0]  # the failed solve: DBL_MAX trials until lambda outweighs H
    assert neg["trials"][0] > neg["iterations"][0] and neg["chi2"][0] < 0


@pytest.mark.parametrize("name", ["63_mixed_25", "300_mono_25", "300_stereo_25", "1000_mixed_25", "257_mixed_0"])
def test_a_known_pose_is_recovered_within_its_noise(cases, both, name):
    """A start off by up to 3 degrees / 5 cm with 25 % gross outliers comes back to the true pose, within its noise.  The bound is the
    estimator's own covariance at the TRUE pose: weighted least squares with weights W = invSigma2 on observations of noise sigma has
    C = (J^T W J)^-1 (J^T W sigma^2 W J) (J^T W J)^-1 over the edges that are not gross outliers (Jacobians from the g2o-form).  Each of the
    six components of log(T_est T_true^-1) must lie within 6 standard deviations; sigma is the case's noise plus 1e-3 px for the float32
    rounding of map points and observations (6e-8 relative of 8 m seen from 0.5 m is 5e-4 px; an observation's ulp is 6e-5 px)."""
    c, (res, flags, g) = cases[name], both[name]
    E = g["edges"]
    cam = pr.Cam(c["camera"])
    true = (gf.normalized(gf.quat_from_matrix(c["R_true"])), c["t_true"])
    pc_true, _, _ = gf.errors(true, cam, E)
    J = gf.jacobians(pc_true, cam, E)
    clean = ~np.isin(E.feat, c["gross"])
    sigma = c["noise"] + 1e-3
    A = np.einsum("nra,n,nrb->ab", J[clean], E.w[clean], J[clean])
    B = np.einsum("nra,n,nrb->ab", J[clean], (E.w[clean] * sigma) ** 2, J[clean])
    std = np.sqrt(np.diag(np.linalg.inv(A) @ B @ np.linalg.inv(A)))
    R, t = np.asarray(res["Rt"][:9]).reshape(3, 3), np.asarray(res["Rt"][9:])
    dR = R @ c["R_true"].T
    err = np.concatenate([0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]), t - dR @ c["t_true"]])
    start = c["camera"]["Rcw"].astype(np.float64).reshape(3, 3) @ c["R_true"].T
    print(f"{name}: noise {c['noise']:.3f} px, inliers {int(res['n_inliers'])} of {E.n}, start {math.degrees(math.acos((np.trace(start) - 1) / 2)):.2f} deg off; "
          f"error / std per component: {np.round(np.abs(err) / std, 2)}; std {std}")
    assert (np.abs(err) <= 6.0 * std).all()
    assert (clean.all() or flags[~clean].mean() > 0.9) and flags[clean].mean() < 0.1  # the gross outliers are the outliers


def _edge_features(c):
    return pr.gather_edges(c["kps"], c["u_right"], c["match"], c["pos"], c["inv_sigma2"], c["count"])[0].feat


def test_the_header_as_a_plain_program_equals_the_restatement(tmp_path, cases, both):
    exe = str(tmp_path / "pose_core_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "host_pose", "pose_core_main.cc")], check=True)
    names = ["65_mixed_25", "1000_stereo_25", "zero_depth_mono"]
    paths = []
    for name in names:
        c, E = cases[name], both[name][2]["edges"]
        rec = np.zeros(E.n, np.dtype([("f", "<f4", (7,)), ("feat", "<i4")]))
        rec["f"] = np.stack([E.u, E.v, E.ur, E.X, E.Y, E.Z, E.w], 1).astype(np.float32)
        rec["feat"] = E.feat
        cam = c["camera"]
        paths.append(str(tmp_path / f"{name}.bin"))
        with open(paths[-1], "wb") as f:
            f.write(struct.pack("<i", E.n) + np.concatenate([cam["Rcw"], cam["tcw"], [cam[k] for k in ("fx", "fy", "cx", "cy", "mbf")]]).astype(np.float32).tobytes()
                    + rec.tobytes())
    out = subprocess.run([exe] + paths, check=True, capture_output=True, text=True).stdout
    blocks = out.split("case ")[1:]
    assert len(blocks) == 3
    for name, block in zip(names, blocks):
        res, flags, _ = both[name]
        lines = block.split("\n")
        head = lines[1].split()
        assert (int(head[1]), int(head[3])) == (int(res["n_inliers"]), int(res["rounds"])), name
        for key, field, dtype in (("Rt", "Rt", np.float64), ("Tcw", "Tcw", np.float32), ("Ow", "Ow", np.float32)):
            got = np.array([float.fromhex(l.split()[1]) for l in lines if l.startswith(key + " ")], dtype)
            assert pc.same_bits(got, res[field]), (name, key)
        rounds = [l.split() for l in lines if l.startswith("round ")]
        assert [int(r[1]) for r in rounds] == list(res["iterations"]) and [int(r[2]) for r in rounds] == list(res["trials"]), name
        assert pc.same_bits(np.array([float.fromhex(r[3]) for r in rounds]), res["lambda"]), name
        assert pc.same_bits(np.array([float.fromhex(r[4]) for r in rounds]), res["chi2"]), name
        assert [l for l in lines if l.startswith("outlier ")][0][8:] == "".join("1" if v else "0" for v in flags), name


def test_the_c_entries_reject_bad_arguments_without_a_device(pkg):
    """validation comes before the device (and before the handle is looked into: a zeroed buffer stands in for it)"""
    L = pkg.lib()
    fake = C.create_string_buffer(1024)
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p).value
    off = np.array([0, 5], np.int32)
    cams, sig = np.zeros(1, pkg.POSE_CAMERA_DTYPE), np.ones(8, np.float32)

    def call(handle=fake, **kw):
        a = dict(d_kps=p, d_u_right=None, d_counts=p, d_match=p, d_points=p, point_stride=12, flags_offset=-1, has_obs_bit=0,
                 point_off=off.ctypes.data, cameras=cams.ctypes.data, inv_level_sigma2=sig.ctypes.data, d_outlier=p, d_result=p, n_frames=1,
                 capacity=16, n_levels=8, clear_outliers=0)
        a.update(kw)
        s = pkg.PoseOptimization(**a)
        return L.amos_match_pose_optimization_batch_device(handle, C.byref(s))
    assert call(handle=None) == -1 and L.amos_match_pose_optimization_batch_device(fake, None) == -1
    for field in ("d_kps", "d_counts", "d_match", "d_points", "point_off", "cameras", "inv_level_sigma2", "d_outlier", "d_result"):
        assert call(**{field: None}) == -1, field
    for kw in (dict(n_frames=0), dict(capacity=0), dict(capacity=65537), dict(n_levels=0), dict(n_levels=17), dict(point_stride=8),
               dict(point_stride=14), dict(flags_offset=8), dict(flags_offset=10, point_stride=16), dict(flags_offset=12), dict(flags_offset=-2),
               dict(clear_outliers=2)):
        assert call(**kw) == -1, kw
    down, neg = np.array([3, 2], np.int32), np.array([-1, 2], np.int32)
    assert call(point_off=down.ctypes.data) == -1 and call(point_off=neg.ctypes.data) == -1
    assert b"amos_match_pose_optimization_batch_device" in L.amos_last_error()
    kp, res = np.zeros(4, pkg.KP_DTYPE), np.zeros(1, pkg.POSE_RESULT_DTYPE)
    m, o, xyz = np.zeros(4, np.int32), np.zeros(4, np.uint8), np.zeros((2, 3), np.float32)

    def host(handle=fake, kps=kp, n=4, match=m, pts=xyz, n_points=2, cam=cams, sigma=sig, n_levels=8, clear=0, outlier=o, result=res):
        g = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.amos_match_pose_optimization(handle, g(kps), None, n, g(match), g(pts), None, n_points, g(cam), g(sigma), n_levels, clear,
                                              g(outlier), g(result))
    assert host(handle=None) == -1 and host(kps=None) == -1 and host(match=None) == -1 and host(outlier=None) == -1 and host(pts=None) == -1
    assert host(cam=None) == -1 and host(sigma=None) == -1 and host(result=None) == -1 and host(n=-1) == -1 and host(n=65537) == -1
    assert host(n_points=-1) == -1 and host(n_levels=0) == -1 and host(n_levels=17) == -1 and host(clear=3) == -1
