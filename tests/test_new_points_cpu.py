"""The new-map-point entry without a GPU: the host compilation of amos-slam_amd/csrc/amos_new_points_core.h against
tests/new_points_restatement.py bit for bit (every verdict, every x3D byte, every stats field), amos_kf_geometry_from_poses against
kf_search_cases.geometry, the restatement's triangulation against an independent float64 SVD, the cases' own checks, the core as a
stand-alone program under -fsanitize=address,undefined, and the C entries' argument refusals."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import host_new_points_binding as hnb
import kf_search_cases as kc
import new_points_cases as nc
import new_points_restatement as nr
import pnp_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1
MAX_LEVELS = 16
f32 = np.float32

# The restatement's x3D (the eigenvector of the smallest eigenvalue of A^T A formed in double from the float32 A, rounded to float32,
# divided in float32) against numpy.linalg.svd of the same float32 A in float64, over every TRIANGULATED match of the random cases: the
# largest |difference| / |x3D| measured, and the bound: eight times it, rounded up to a power of ten.  (Two float32 roundings of the
# components and one of 1 / w account for about 3 * 2^-24 = 1.8e-7.)
SVD_MEASURED = 1.04e-07  # over 84 matches (test_restatement_against_a_float64_svd prints it; also in DESIGN.md section 7)
SVD_BOUND = 1e-06
# F of amos_kf_geometry_from_poses against kc.geometry (float64, rounded once) after dividing each by its largest |entry|: three float32
# gemms and the float32 K^-1 entries behind entries of size 1: a few float32 epsilons (6e-8 each) per entry, times the cancellation of
# K^-T [t]x R K^-1's largest terms (cx / fx, cy / fy of order 1 against entries of order 1e-3 .. 1): 1e-4 of the largest entry.
F_BOUND = 1e-4


def all_cases():
    cases = dict(nc.hand_cases())
    cases.update(nc.random_cases())
    return cases


def test_the_cases_do_what_they_are_named_for():
    hist = nc.check_cases()
    print("verdicts over the random cases:", dict(zip(nr.VERDICT_NAMES, hist.tolist())))


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_host_compilation_of_the_core_equals_the_restatement(name):
    case = all_cases()[name]
    for with_raw, with_right in ((True, True), (False, True), (True, False)):
        a = hnb.pack(case, with_raw=with_raw, with_right=with_right)
        new, verdict, stats = hnb.core(a)
        want_new, want_verdict, want_stats = hnb.expected(hnb.stripped(case, with_raw, with_right), a["capacity"])
        assert verdict.tobytes() == want_verdict.tobytes(), (name, with_raw, with_right)
        assert stats.tobytes() == want_stats.tobytes(), (name, with_raw, with_right)
        assert new.tobytes() == want_new.tobytes(), (name, with_raw, with_right)


def test_a_disabled_pair_and_the_claim_rule_behind_it():
    """pair 0 disabled: zero stats, a row of -1, and what it would have accepted is not claimed in the later pairs"""
    case = dict(nc.hand_cases()["claimed"], enabled=[0, 1, 1])
    a = hnb.pack(case)
    new, verdict, stats = hnb.core(a)
    want = hnb.expected(case, a["capacity"])
    assert (new.tobytes(), verdict.tobytes(), stats.tobytes()) == tuple(w.tobytes() for w in want)
    assert stats[0].tobytes() == bytes(64) and (verdict[0] == -1).all()
    assert verdict[1, :2].tolist() == [nr.REPROJECTION_1, nr.TRIANGULATED] and verdict[2, :2].tolist() == [nr.TRIANGULATED, nr.CLAIMED]


def test_unrolled_jacobi_equals_jacobi_sym_bit_for_bit():
    """jacobi_sym4 against pnp::jacobi_sym(., ., 4) in one compilation, and both against the restatement: A^T A of the random cases'
    triangulation matrices, random symmetric matrices, and the degenerate ones (zero, diagonal, equal eigenvalues, a NaN)"""
    rng = np.random.default_rng(4)
    mats = []
    for _ in range(200):
        M = rng.normal(size=(4, 4)) * 10.0 ** rng.integers(-3, 4)
        mats.append(M.T @ M if rng.random() < 0.5 else M + M.T)
    mats += [np.zeros((4, 4)), np.diag([3.0, 1.0, 1.0, 2.0]), np.eye(4), np.ones((4, 4)), np.diag([1.0, 2.0, 3.0, 4.0]) + 1e-300]
    bad = np.eye(4)
    bad[1, 2] = bad[2, 1] = np.nan
    mats.append(bad)
    for k, S in enumerate(mats):
        S = (S + S.T) / 2
        Su, Vu = hnb.jacobi(S, "unrolled")
        Sg, Vg = hnb.jacobi(S, "generic")
        assert Su.tobytes() == Sg.tobytes() and Vu.tobytes() == Vg.tobytes(), k
        with np.errstate(all="ignore"):
            lam, V = pr.jacobi_sym(S)
        assert np.array(lam).tobytes() == np.diag(Su).copy().tobytes() and np.ascontiguousarray(V).tobytes() == Vu.tobytes(), k


def test_w_zero_and_distance_zero_on_the_core_functions():
    # A with a zero first column: the null vector is e1 exactly, w == 0
    A = np.array([[0, 1, 2, 3], [0, -2, 1, 0.5], [0, 0.25, -3, 1], [0, 4, 1, -2]], f32)
    v = hnb.null_vector(A)
    assert v.tobytes() == nr.null_vector4(A).tobytes() == np.array([1, 0, 0, 0], f32).tobytes()
    assert hnb.dehomogenise(v) is None and nr.dehomogenise(v) is None
    w = np.array([2, -4, 6, 0.5], f32)
    assert hnb.dehomogenise(w).tobytes() == nr.dehomogenise(w).tobytes() == np.array([4, -8, 12], f32).tobytes()
    # x3D equal to a camera centre: zero distance, on either side
    c1, c2 = nc.hand_cam((0.25, -1.0, 2.0)), nc.hand_cam((0.5, 0, 0))
    sf = nc.HAND_LEVELS[0]
    for cams, X in (((c1, c2), c1["Ow"]), ((c2, c1), c1["Ow"])):
        assert hnb.scale_gate(*cams, 0, 0, sf, X) == nr.scale_gate(*cams, 0, 0, sf, X) == nr.DISTANCE_ZERO
    assert hnb.scale_gate(c1, c2, 0, 0, sf, [0.3, 0.1, 5.0]) == nr.scale_gate(c1, c2, 0, 0, sf, np.array([0.3, 0.1, 5.0], f32)) == 0
    # a NaN fails the gate it meets
    nan = np.array([np.nan, 0, 1], f32)
    assert hnb.scale_gate(c1, c2, 0, 0, sf, nan) == nr.scale_gate(c1, c2, 0, 0, sf, nan) == nr.SCALE


def test_cos_of_twice_atan2_restated():
    """(d^2 - h^2) / (d^2 + h^2) is cos(2 atan2(h, d)) in every quadrant, and 1 at the origin"""
    rng = np.random.default_rng(9)
    for _ in range(300):
        mb, d = f32(rng.normal() * 0.2), f32(rng.normal() * 10.0 ** rng.integers(-2, 3))
        got = hnb.cos_stereo(mb, d)
        assert got.tobytes() == nr.cos_stereo_parallax(mb, d).tobytes()
        assert abs(float(got) - np.cos(2 * np.arctan2(float(mb / f32(2)), float(d)))) <= 2e-7
    assert hnb.cos_stereo(0.0, 0.0) == 1.0 and nr.cos_stereo_parallax(0.0, 0.0) == 1.0
    assert np.isnan(hnb.cos_stereo(0.08, np.nan)) and np.isnan(nr.cos_stereo_parallax(0.08, np.nan))


def _poses():
    rng = np.random.default_rng(12)
    out = []
    for _ in range(20):
        R1, R2 = kc._rot(*rng.normal(size=3) * 0.3), kc._rot(*rng.normal(size=3) * 0.3)
        out.append((nr.camera(R1, rng.normal(size=3), nc.K_HAND, 0.08, 40.0), nr.camera(R2, rng.normal(size=3), (520.0, 510.0, 300.0, 250.0), 0.1, 52.0)))
    return out


def test_geometry_from_poses(pkg):
    """the library's host compilation == the harness's == the restatement, bit for bit, on general poses; against kc.geometry on the poses
    behind the random pairs and the hand geometries: F within F_BOUND of its largest entry, the epipole with =="""
    for c1, c2 in _poses() + [(nc.hand_cam(), nc.hand_cam((0.01, 0, 0))), (nc.hand_cam(), nc.hand_cam((0.08, 0, 0))), (nc.hand_cam(), nc.hand_cam((0.0801, 0, 0)))]:
        want, want_ok = nr.pair_geometry(c1, c2)
        for got, ok in (pkg.kf_geometry_from_poses(c1, c2), hnb.geometry(c1, c2)):
            assert got.tobytes() == want.tobytes() and ok == want_ok
    assert not nr.pair_geometry(nc.hand_cam(), nc.hand_cam((0.01, 0, 0)))[1] and nr.pair_geometry(nc.hand_cam(), nc.hand_cam((0.0801, 0, 0)))[1]
    worst = 0.0
    K_hand = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]])
    for K, (R12, t12), mb in [(kc.camera(640, 480), nc.MOTIONS[k], nc.MB) for k in nc.RANDOM_KINDS] + \
                             [(K_hand, (np.eye(3), np.array(t)), 0.08) for t in ([1.0, 0, 0], [0, 0, 1.0], [0.3, -0.2, 0.1])]:
        c1, c2 = nc.pose_cameras(K, R12, t12, mb)
        got, ok = pkg.kf_geometry_from_poses(c1, c2)
        want = kc.geometry(K, R12, t12)
        a, b = got["f12"].astype(np.float64), want["f12"].astype(np.float64)
        err = np.abs(a / np.abs(a).max() - b / np.abs(b).max()).max()
        worst = max(worst, err)
        assert ok and err <= F_BOUND
        assert np.array_equal(got["ex"], want["ex"], equal_nan=True) and np.array_equal(got["ey"], want["ey"], equal_nan=True)  # == (an epipole at infinity: NaN)
    print(f"F against float64, largest difference after normalisation: {worst:.3g} (bound {F_BOUND:g})")
    for name, case in nc.random_cases().items():  # the cases' own geometry record is what their cameras give
        g = pkg.kf_geometry_from_poses(case["cams"][0], case["cams"][1])[0]
        assert np.array_equal(g["ex"], case["geo"]["ex"], equal_nan=True) and np.array_equal(g["ey"], case["geo"]["ey"], equal_nan=True), name


def test_restatement_against_a_float64_svd():
    """every TRIANGULATED match of the random cases; none is left out"""
    worst, count = 0.0, 0
    for name, case in nc.random_cases().items():
        sides, cams, (sf, sg) = case["sides"], case["cams"], case["levels"]
        for (s1, s2), row in zip(case["pairs"], case["match"]):
            for i, m in enumerate(row):
                if m < 0:
                    continue
                tr = {}
                v, X = nr.triangulate_match(cams[s1], cams[s2], nr.feature(sides[s1], i), nr.feature(sides[s2], int(m)), sf, sg, trace=tr)
                if "A" not in tr or v == nr.W_ZERO or v == nr.OCTAVE:
                    continue
                vt = np.linalg.svd(tr["A"].astype(np.float64).reshape(4, 4))[2][3]
                ref = vt[:3] / vt[3]
                rel = np.abs(X.astype(np.float64) - ref).max() / np.abs(ref).max()
                worst, count = max(worst, rel), count + 1
                assert rel <= SVD_BOUND, (name, i, rel)
    print(f"restatement against numpy.linalg.svd: {count} matches, largest relative difference {worst:.4g} (recorded {SVD_MEASURED:g}, bound {SVD_BOUND:g})")
    assert count >= 50 and worst <= SVD_MEASURED * 1.0000001


def test_the_known_point_is_recovered_on_noise_free_matches():
    rng = np.random.default_rng(3)
    c1 = nc.hand_cam()
    for k in range(40):
        c2 = nc.hand_cam(rng.normal(size=3) * [0.4, 0.4, 0.1], kc._rot(*rng.normal(size=3) * 0.05))
        P = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 8)])
        if np.linalg.norm(c2["Ow"]) < 0.2:
            continue
        sides = nc._two(P, c1, c2)
        v, X = nr.triangulate_match(c1, c2, nr.feature(sides[0], 0), nr.feature(sides[1], 0), *nc.HAND_LEVELS)
        assert v == nr.TRIANGULATED, k
        # a pixel rounded to float32 (3e-5 px) moves the point by depth^2 / (f * baseline) * that: below 1e-3 here
        assert np.abs(X.astype(np.float64) - P).max() < 2e-3, (k, X, P)


def test_the_core_as_a_sanitized_plain_program_equals_the_restatement(tmp_path):
    """Host code in a stand-alone program with its own main, compiled with -fsanitize=address,undefined: it must end clean with the
    restatement's outputs for the hand cases and one random case."""
    exe = str(tmp_path / "new_points_core_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "host_new_points", "new_points_core_main.cc")], check=True)
    cases = dict(nc.hand_cases())
    cases["forward_5"] = nc.random_case(5, "forward")
    cases["disabled"] = dict(nc.hand_cases()["claimed"], enabled=[1, 0, 1])
    paths, wants = [], []
    for name, case in sorted(cases.items()):
        a = hnb.pack(case, pad=0 if name == "triangulated" else 3)
        paths.append(str(tmp_path / f"{name}.bin"))
        hnb.write_case_file(paths[-1], a)
        wants.append(hnb.expected(case, a["capacity"]))
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    blocks = run.stdout.strip().split("case ")[1:]
    assert len(blocks) == len(paths)
    for block, (new, verdict, stats) in zip(blocks, wants):
        lines = block.strip().split("\n")[1:]
        for p in range(len(stats)):
            assert [int(x) for x in lines.pop(0).split()[1:]] == np.frombuffer(stats[p].tobytes(), np.int32).tolist()
            assert [int(x) for x in lines.pop(0).split()[1:]] == verdict[p].tolist()
            for e in range(int(stats[p]["n_new"])):
                r = new[p, e]
                bits = np.array([r["x"], r["y"], r["z"]], f32).view(np.uint32).tolist()
                assert [int(x) for x in lines.pop(0).split()[1:]] == [int(r["idx1"]), int(r["idx2"])] + bits + [int(r["verdict"])]
        assert not lines


def struct_bytes(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.split()[0] in ("float", "int32_t"), decl
        for item in decl.split(None, 1)[1].split(","):
            dims = re.findall(r"\[(\w+)\]", item)
            n += int(np.prod([13 if d == "AMOS_NEW_POINT_VERDICTS" else int(d) for d in dims])) if dims else 1
    return 4 * n


def test_exports_and_struct_sizes(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    for name in ("amos_match_new_points_batch_device", "amos_match_new_points", "amos_kf_geometry_from_poses"):
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "amos_frontend.h")).read()
    for name, dt, mine in (("amos_kf_camera", pkg.KF_CAMERA_DTYPE, nr.KF_CAMERA), ("amos_new_point", pkg.NEW_POINT_DTYPE, nr.NEW_POINT),
                           ("amos_new_points_stats", pkg.NEW_POINTS_STATS_DTYPE, nr.NEW_POINTS_STATS)):
        assert struct_bytes(header, name) == dt.itemsize == mine.itemsize and dt == mine, name
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct amos_new_points \{(.*?)\} amos_new_points;", header, re.S).group(1), flags=re.S)
    assert C.sizeof(pkg.NewPoints) == 8 * len(re.findall(r"\*", body)) + 4 * 4
    for k, name in enumerate(nr.VERDICT_NAMES):
        assert re.search(r"#define AMOS_NEW_POINT_%s %d\b" % (name, k), header) and getattr(pkg, "NEW_POINT_" + name) == k, name
    assert (pkg.NEW_POINTS_BAD_MATCH, pkg.NEW_POINTS_BAD_OCTAVE, pkg.NEW_POINTS_BAD_SLOT) == (nr.BAD_MATCH, nr.BAD_OCTAVE, nr.BAD_SLOT)


def test_the_c_entries_reject_bad_arguments_without_a_device(pkg):
    """validation comes before the device (and before the handle is looked into: a zeroed buffer stands in for it)"""
    L = pkg.lib()
    fake = C.create_string_buffer(4096)
    buf = np.zeros(1 << 16, np.uint8)
    keep = []
    cams = np.stack([nc.hand_cam(), nc.hand_cam((0.5, 0, 0)), nc.hand_cam((0, 0.5, 0))])

    def cams_with(k, field, value):
        c = cams.copy()
        if c[field].ndim > 1:
            c[field][k, 0] = value
        else:
            c[field][k] = value
        return c

    def struct_of(**kw):
        p = buf.ctypes.data
        c = np.ascontiguousarray(kw.pop("cams", cams), nr.KF_CAMERA)
        p1, p2 = np.array(kw.pop("p1", [0, 0]), np.int32), np.array(kw.pop("p2", [1, 2]), np.int32)
        en = kw.pop("en", None)
        en = None if en is None else np.array(en, np.uint8)
        keep.extend([c, p1, p2, en])
        d = dict(d_kps=p, d_kps_raw=None, d_counts=p, d_u_right=p, d_depth=p, d_pairs_1=p, d_pairs_2=p, d_match12=p, d_scale_factors=p, d_level_sigma2=p,
                 cameras=c.ctypes.data, pairs_1=p1.ctypes.data, pairs_2=p2.ctypes.data, enabled=None if en is None else en.ctypes.data, d_new=p + 8192,
                 d_verdict=None, d_stats=p + 4096, n_frames=3, n_pairs=2, capacity=64, n_levels=8)
        d.update(kw)
        return pkg.NewPoints(**d)

    bad = [struct_of(**{k: None}) for k in ("d_kps", "d_counts", "d_depth", "d_pairs_1", "d_pairs_2", "d_match12", "d_scale_factors", "d_level_sigma2",
                                            "cameras", "pairs_1", "pairs_2", "d_new", "d_stats")]
    bad += [struct_of(n_pairs=0), struct_of(n_pairs=65), struct_of(n_frames=0), struct_of(capacity=0), struct_of(capacity=65537), struct_of(n_levels=0),
            struct_of(n_levels=MAX_LEVELS + 1), struct_of(p1=[0, 3]), struct_of(p2=[1, -1]), struct_of(p2=[1, 1]), struct_of(p2=[2, 2], en=[1, 1]),
            struct_of(cams=cams_with(0, "fx", 0.0)), struct_of(cams=cams_with(2, "fy", -1.0)), struct_of(cams=cams_with(1, "Rcw", np.nan)),
            struct_of(cams=cams_with(0, "Ow", np.inf)), struct_of(cams=cams_with(1, "mbf", np.nan))]
    for k, s in enumerate(bad):
        assert L.amos_match_new_points_batch_device(fake, C.byref(s)) == ERR_INVALID, k
        assert b"amos_match_new_points_batch_device" in L.amos_last_error(), k
    assert L.amos_match_new_points_batch_device(None, C.byref(struct_of())) == ERR_INVALID
    assert L.amos_match_new_points_batch_device(fake, None) == ERR_INVALID
    assert L.amos_kf_geometry_from_poses(None, cams.ctypes.data, buf.ctypes.data) == ERR_INVALID
    assert L.amos_kf_geometry_from_poses(cams.ctypes.data, cams.ctypes.data, None) == ERR_INVALID
    # the host form
    k1, k2 = nc.random_case(5, "forward")["sides"][:2]
    cam = nc.random_case(5, "forward")["cams"]
    sf, sg = nc.random_case(5, "forward")["levels"]

    stand_in = types.SimpleNamespace(h=fake, L=L, _bow_view=pkg.OrbMatcher._bow_view)  # OrbMatcher.new_points on a handle that is never looked into

    def host(k1=k1, k2s=(k2,), cam1=cam[0], cams2=(cam[1],), sf=sf, sg=sg):
        return pkg.OrbMatcher.new_points(stand_in, kc.with_csr(k1), [kc.with_csr(k) for k in k2s], cam1, np.stack(cams2) if len(cams2) else np.zeros(0, nr.KF_CAMERA), sf, sg)
    for kw in (dict(k2s=(), cams2=()), dict(k1=dict(k1, depth=None)), dict(k2s=(dict(k2, depth=None),)), dict(sf=np.ones(17, f32), sg=np.ones(17, f32)),
               dict(k2s=(dict(k2, fv={5: [0, len(k2["desc"])]}),)), dict(k2s=(k2,) * 65, cams2=(cam[1],) * 65)):
        with pytest.raises(pkg.AmosError, match="rc=-1"):
            host(**kw)
    # every neighbour fails the baseline gate: zero stats and no device
    near = cam[0].copy()
    rows, stats = host(cams2=(near,))
    assert len(rows[0]) == 0 and stats.tobytes() == bytes(64)
