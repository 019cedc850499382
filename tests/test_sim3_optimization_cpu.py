"""CPU: the loop-closing Sim3 optimisation without a GPU.  The host compilation of amos-slam_amd/csrc/amos_sim3_opt_core.h must equal the
restatement (tests/sim3_optimization_restatement.py) bit for bit in every result field and row entry over the grid the GPU tests use and
over hand-made cases; the restatement must agree with an independent form written from the g2o text (tests/sim3_optimization_g2o_form.py);
exp_ must keep its recorded accuracy; the exports, the record sizes and the C entries' argument checks; the core as a stand-alone program
under -fsanitize=address,undefined."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import host_sim3_optimize_binding as hso
import sim3_optimization_cases as sc
import sim3_optimization_g2o_form as g2
import sim3_optimization_restatement as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, MAX_LEVELS = -1, 16  # AMOS_ERR_INVALID, AMOS_MAX_LEVELS (include/amos_frontend.h)
# The largest difference between the restatement's and the g2o form's Sim3 (any of q, t, s) over the grid, measured on the CPU: 2.2e-6
# (n19_fix0_out25; the central difference divides rounding noise by 2e-9, and five to fifteen iterations carry it on).  The test allows ten
# times that: the margin covers another libm.
G2O_FORM_MEASURED = 2.2e-6


@pytest.fixture(scope="module")
def shared():
    return sc.shared()


def core_equals(s, want=None, what=""):
    res, row = sc.expected(s) if want is None else want
    got = hso.optimize("core", s, sc.INV_SIGMA2)
    diff = [f for f in so.RESULT.names if np.asarray(got["result"][f]).tobytes() != np.asarray(res[f]).tobytes()]
    assert not diff and got["ret"] == res["n_inliers"], (what, diff, got["result"], res)
    assert got["result"].tobytes() == res.tobytes() and np.array_equal(got["row"], row), what
    return res, row


def test_host_compilation_of_the_core_equals_the_restatement(shared):
    grid, want = shared
    assert [s["n"] for _, s in grid][::4] == list(sc.GRID_COUNTS) and len(grid) == 48
    for (name, s), w in zip(grid, want):
        res, row = core_equals(s, w, name)
        assert res["n_correspondences"] == s["n"], name
        print(name, "bad first", res["n_bad_first"], "inliers", res["n_inliers"], "iterations", res["iterations"].tolist(), "trials", res["trials"].tolist())


def test_hand_made_cases(shared):
    grid, want = shared
    by_name = {n: (s, w) for (n, s), w in zip(grid, want)}
    # nBad == 0: five more iterations at the most; nBad > 0: ten
    res = by_name["n64_fix0_out0"][1][0]
    assert res["n_bad_first"] == 0 and res["rounds"] == 2 and res["iterations"][1] <= 5 and res["n_inliers"] == 64
    s, (res, row) = by_name["n64_fix0_out25"]
    assert res["n_bad_first"] == 16 and res["rounds"] == 2 and res["iterations"][1] > 5 and res["n_inliers"] == 48
    assert np.array_equal(row == -1, (s["row"] == -1) | s["is_outlier"])
    # nCorrespondences - nBad < 10 after the first pass: 0, the entries cleared, the Sim3 as it came
    s, (res, row) = by_name["n11_fix0_out25"]
    assert res["n_bad_first"] == 3 and res["rounds"] == 1 and res["n_inliers"] == 0 and (row[s["is_outlier"]] == -1).all()
    assert res["R12"].tobytes() == s["pair"]["R12"].tobytes() and res["t12"].tobytes() == s["pair"]["t12"].tobytes() and res["s12"] == s["pair"]["s12"]
    assert res["q"].tolist() == so.pose_from_floats(s["pair"]["R12"], s["pair"]["t12"], s["pair"]["s12"], 0).q
    # fewer than 10 on entry; none at all
    res = by_name["n9_fix1_out0"][1][0]
    assert res["n_correspondences"] == 9 and res["rounds"] == 1 and res["n_inliers"] == 0
    for empty in (sc.scene(0, 0, extra=False), dict(by_name["n20_fix0_out0"][0], row=np.full(len(by_name["n20_fix0_out0"][0]["row"]), -1, np.int32))):
        res, row = core_equals(empty, what="empty")
        assert res["n_correspondences"] == 0 and res["rounds"] == 0 and res["n_inliers"] == 0 and res["Scw"][15] == 1.0
    # entries of -2 and out-of-range entries are no correspondences; skip flags on either side; an octave outside the table
    s = dict(by_name["n20_fix1_out0"][0])
    base = sc.expected(s)[0]
    feats = np.nonzero(s["row"] >= 0)[0]
    s["row"], s["pts1"], s["pts2"], s["kps1"], s["kps2"] = s["row"].copy(), s["pts1"].copy(), s["pts2"].copy(), s["kps1"].copy(), s["kps2"].copy()
    s["row"][feats[0]], s["row"][feats[1]], s["row"][feats[2]] = -2, len(s["kps2"]), -7
    s["pts1"]["flags"][feats[3]] = so.POINT_SKIP
    s["pts2"]["flags"][s["row"][feats[4]]] = so.POINT_SKIP
    res, row = core_equals(s, what="entries")
    assert res["n_correspondences"] == base["n_correspondences"] - 5 and res["status"] == 0
    assert row[feats[0]] == -2 and row[feats[1]] == len(s["kps2"]) and row[feats[2]] == -7 and row[feats[3]] >= 0 and row[feats[4]] >= 0
    s["kps1"]["octave"][feats[5]], s["kps2"]["octave"][s["row"][feats[6]]] = sc.N_LEVELS, -1
    res, row = core_equals(s, what="octaves")
    assert res["n_correspondences"] == base["n_correspondences"] - 7 and res["status"] == so.STATUS_OCTAVE
    # an exact optimum: every residual 0.0 at the start, b = 0, rho == 0 stops the first iteration of both optimisations
    for fix in (0, 1):
        s = sc.exact_scene(fix_scale=fix)
        res, row = core_equals(s, what="exact")
        assert res["iterations"].tolist() == [1, 1] and res["trials"].tolist() == [1, 1] and res["chi2"].tolist() == [0.0, 0.0]
        assert res["n_inliers"] == s["n"] and np.array_equal(row, s["row"]) and res["s"] == 1.0 and res["q"].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_restatement_agrees_with_the_form_written_from_the_g2o_text(shared):
    """n_inliers, n_bad_first and every cleared entry agree; the Sim3 agrees within ten times the measured 2.2e-6 (see G2O_FORM_MEASURED).
    First: no edge's chi2 at a classification lies within a relative 1e-3 of th2 in the restatement, so a flag cannot hinge on rounding."""
    grid, _ = shared
    worst = 0.0
    for name, s in grid:
        Cs, status = so.gather(s["kps1"], s["pts1"], s["cam1"], s["kps2"], s["pts2"], s["cam2"], s["row"], sc.INV_SIGMA2)
        trace = []
        res, bad = so.optimize_corrs(Cs, s["pair"], s["cam1"], s["cam2"], status, trace)
        for tr in trace:
            for c in (tr["c12"], tr["c21"]):
                assert (np.abs(c[tr["active"]] / sc.TH2 - 1.0) > 1e-3).all(), (name, "an edge within 1e-3 of th2")
        g = g2.optimize(Cs, s["pair"], s["cam1"], s["cam2"])
        assert g["n_inliers"] == res["n_inliers"] and g["n_bad_first"] == res["n_bad_first"] and np.array_equal(g["bad"], bad), name
        d = max(np.abs(g["q"] - res["q"]).max(), np.abs(g["t"] - res["t"]).max(), abs(g["s"] - res["s"]))
        print(name, "difference", d)
        worst = max(worst, d)
    print("largest difference", worst)
    assert worst <= 10 * G2O_FORM_MEASURED


def ulps(a, b):
    return abs(a - b) / math.ulp(b)


def test_exp_accuracy():
    xs = list(np.linspace(-1.0, 1.0, 200001)) + [1e-9, -1e-9]
    worst = max(ulps(so.exp_(float(x)), math.exp(float(x))) for x in xs)
    print("exp_: worst error against the C library", worst, "ulp")
    assert worst <= so.EXP_ULP + 1.0
    assert so.exp_(0.0) == 1.0 and hso.exp_(0.0) == 1.0
    header = open(os.path.join(ROOT, "amos-slam_amd", "csrc", "amos_sim3_opt_core.h")).read()
    assert f"kExpUlp = {so.EXP_ULP}" in header
    for x in (0.0, 1e-9, -1e-9, 0.3, -0.7, 1.0, 5.5, -20.25, 700.0, -740.0, 1e4, -1e4):
        assert hso.exp_(x) == so.exp_(x), x
    assert math.isnan(hso.exp_(math.nan))


def test_exports_and_struct_sizes(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    for name in ("amos_match_sim3_optimize_batch_device", "amos_match_sim3_optimize"):
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    source = open(os.path.join(ROOT, "amos-slam_amd", "csrc", "amos_sim3_opt.hip")).read()
    assert pkg.SIM3_OPT_PAIR_DTYPE.itemsize == so.PAIR.itemsize == 64 and "sizeof(amos_sim3_opt_pair) == 64" in source
    assert pkg.SIM3_OPT_RESULT_DTYPE.itemsize == so.RESULT.itemsize == 256 and "sizeof(amos_sim3_opt_result) == 256" in source
    assert pkg.SIM3_OPT_RESULT_DTYPE == so.RESULT and pkg.SIM3_OPT_PAIR_DTYPE == so.PAIR
    assert C.sizeof(pkg.Sim3Optimize) == 8 * 12 + 4 * 4


def test_the_c_entries_reject_bad_arguments_without_a_device(pkg):
    """validation comes before the device (and before the handle is looked into: a zeroed buffer stands in for it)"""
    L = pkg.lib()
    fake = C.create_string_buffer(4096)
    buf = np.zeros(1 << 16, np.uint8)
    cams = np.zeros(2, pkg.SIM3_CAMERA_DTYPE)
    cams["fx"] = cams["fy"] = 500.0
    keep = []

    def pairs_of(**kw):
        pr = np.array([pkg.sim3_opt_pair(np.eye(3), [0.1, 0, 0], 1.0)] * 2)
        for k, v in kw.items():
            pr[k][1] = v
        return pr

    def struct_of(**kw):
        pr, cam = kw.pop("pairs", pairs_of()), kw.pop("cameras", cams)
        keep.extend([pr, cam])
        p = buf.ctypes.data
        d = dict(d_kps=p, d_counts=p, d_points=p, cameras=None if cam is None else cam.ctypes.data, d_pairs_1=p, d_pairs_2=p,
                 inv_level_sigma2=sc.INV_SIGMA2.ctypes.data, pairs=None if pr is None else pr.ctypes.data, d_sim3=None, d_match12=p, d_match_out=p,
                 d_result=p, n_frames=2, n_pairs=2, capacity=64, n_levels=8)
        d.update(kw)
        return pkg.Sim3Optimize(**d)

    bad_cam = cams.copy()
    bad_cam["tcw"][1, 2] = np.nan
    nan_R = np.eye(3)
    nan_R[1, 1] = np.nan
    bad = [struct_of(**{k: None}) for k in ("d_kps", "d_counts", "d_points", "cameras", "d_pairs_1", "d_pairs_2", "inv_level_sigma2", "pairs", "d_match12",
                                            "d_match_out", "d_result")]
    bad += [struct_of(n_pairs=0), struct_of(n_frames=0), struct_of(capacity=0), struct_of(capacity=65537), struct_of(n_levels=0),
            struct_of(n_levels=MAX_LEVELS + 1), struct_of(cameras=bad_cam), struct_of(pairs=pairs_of(R12=nan_R.reshape(9))),
            struct_of(pairs=pairs_of(t12=[0, np.inf, 0])), struct_of(pairs=pairs_of(s12=0.0)), struct_of(pairs=pairs_of(s12=-1.0)),
            struct_of(pairs=pairs_of(s12=np.nan)), struct_of(pairs=pairs_of(th2=0.0)), struct_of(pairs=pairs_of(th2=np.nan)),
            struct_of(pairs=pairs_of(th2=np.inf)), struct_of(pairs=pairs_of(fix_scale=2)), struct_of(pairs=pairs_of(fix_scale=-1)),
            struct_of(pairs=pairs_of(enabled=2)), struct_of(pairs=pairs_of(enabled=0, fix_scale=3)),
            struct_of(d_sim3=buf.ctypes.data, pairs=pairs_of(th2=-1.0))]
    for k, s in enumerate(bad):
        assert L.amos_match_sim3_optimize_batch_device(fake, C.byref(s)) == ERR_INVALID, k
    assert L.amos_match_sim3_optimize_batch_device(None, C.byref(struct_of())) == ERR_INVALID
    assert L.amos_match_sim3_optimize_batch_device(fake, None) == ERR_INVALID
    # the host form
    kps, pts = np.zeros(4, pkg.KP_DTYPE), np.zeros(4, pkg.SIM3_POINT_DTYPE)
    row, out, res = np.full(4, -1, np.int32), np.zeros(4, np.int32), np.zeros(1, pkg.SIM3_OPT_RESULT_DTYPE)
    ptr = lambda a: None if a is None else a.ctypes.data

    def host(**kw):
        a = dict(m=fake, kps1=kps, points1=pts, n1=4, kps2=kps, points2=pts, n2=4, cameras=cams, match12=row, sig=sc.INV_SIGMA2, n_levels=8,
                 pair=pairs_of()[:1], out=out, result=res)
        a.update(kw)
        return L.amos_match_sim3_optimize(a["m"], ptr(a["kps1"]), ptr(a["points1"]), a["n1"], ptr(a["kps2"]), ptr(a["points2"]), a["n2"], ptr(a["cameras"]),
                                          ptr(a["match12"]), ptr(a["sig"]), a["n_levels"], ptr(a["pair"]), ptr(a["out"]), ptr(a["result"]))

    one = lambda **kw: pairs_of(**kw)[1:]
    for kw in (dict(m=None), dict(kps1=None), dict(points1=None), dict(kps2=None), dict(points2=None), dict(cameras=None), dict(match12=None),
               dict(sig=None), dict(pair=None), dict(out=None), dict(result=None), dict(n1=-1), dict(n2=65537), dict(n_levels=0),
               dict(n_levels=MAX_LEVELS + 1), dict(cameras=bad_cam), dict(pair=one(s12=0.0)), dict(pair=one(th2=-2.0)), dict(pair=one(fix_scale=5)),
               dict(pair=one(t12=[np.nan, 0, 0]))):
        assert host(**kw) == ERR_INVALID, kw


def write_case(path, s):
    with open(path, "wb") as f:
        f.write(np.array([len(s["kps1"]), len(s["kps2"]), len(sc.INV_SIGMA2), 0], np.int32).tobytes())
        f.write(np.array([s["cam1"], s["cam2"]], so.CAMERA).tobytes())
        f.write(np.array([s["pair"]], so.PAIR).tobytes())
        f.write(sc.INV_SIGMA2.tobytes())
        for k in ("kps1", "pts1", "kps2", "pts2"):
            f.write(np.ascontiguousarray(s[k]).tobytes())
        f.write(np.asarray(s["row"], np.int32).tobytes())


def test_the_core_as_a_sanitized_plain_program_equals_the_restatement(shared, tmp_path):
    """Host code in a stand-alone program with its own main, compiled with -fsanitize=address,undefined: it must end clean with the
    restatement's record and row for two cases (both fix_scale values, with and without gross outliers)."""
    grid, want = shared
    exe = str(tmp_path / "sim3_optimize_core_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "host_sim3_optimize", "sim3_optimize_core_main.cc")], check=True)
    names = [n for n, _ in grid]
    picks = [names.index("n65_fix0_out25"), names.index("n257_fix1_out0")]
    paths = []
    for p in picks:
        paths.append(str(tmp_path / f"case{p}.bin"))
        write_case(paths[-1], grid[p][1])
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    blocks = run.stdout.split("case ")[1:]
    assert len(blocks) == len(picks)
    for blk, p in zip(blocks, picks):
        lines = blk.splitlines()
        res, row = want[p]
        assert int(lines[1]) == res["n_inliers"] and bytes.fromhex(lines[2]) == res.tobytes(), names[p]
        assert [int(v) for v in lines[3].split()] == row.tolist(), names[p]
