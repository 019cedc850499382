"""CPU: the loop-closing Sim3 search without a GPU.  The restatement of ORBmatcher::SearchBySim3 (tests/sim3_search_restatement.py) must equal
the pre-filter of tests/adaptor_prefilter.py fed to the oracle's orc_search_by_sim3 on every pair of the scene the GPU tests use; the host
compilation of amos-slam_amd/csrc/amos_sim3_search_core.h must equal its projections with ==; that scene must hold every case the GPU tests
rely on -- so a pass on the GPU means something; the exports, the struct sizes and the C entries' argument checks; the core as a
stand-alone program under -fsanitize=address,undefined."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import adaptor_prefilter as ap
import host_binding as hb
import host_sim3_search_binding as hsb
import sim3_search_restatement as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ERR_INVALID, MAX_LEVELS = -1, 16  # AMOS_ERR_INVALID, AMOS_MAX_LEVELS (include/amos_frontend.h)
R = ss.REASONS


@pytest.fixture(scope="module")
def shared():
    return ss.shared()


def T_of(cam):
    T = np.eye(4, dtype=f32)
    T[:3, :3], T[:3, 3] = cam["Rcw"].reshape(3, 3), cam["tcw"]
    return T


def test_restatement_equals_prefilter_plus_oracle(ob, shared):
    """Both directions' queries from adaptor_prefilter.sim3_direction (MapPoint::PredictScale in its logf form), the searches and the agreement
    from the oracle.  The two forms of PredictScale must agree on every feature that reaches its window."""
    sc, results = shared
    sf, bounds = sc["sf"], sc["bounds"]
    cam_ns = lambda c: types.SimpleNamespace(fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], min_x=bounds[0], max_x=bounds[1], min_y=bounds[2],
                                             max_y=bounds[3])
    for p, got in enumerate(results):
        a, b = int(sc["slots1"][p]), int(sc["slots2"][p])
        kf1, kf2 = ss.keyframe(sc, a), ss.keyframe(sc, b)
        n1, n2 = len(kf1["kps"]), len(kf2["kps"])
        pr, row = sc["pairs"][p], sc["rows"][p][:n1]
        if n1 == 0 or n2 == 0:  # nothing to hand to the oracle: no feature is accepted on either side
            assert got["stats"]["n_found"] == 0 and (got["match1"] == -1).all() and (got["match2"] == -1).all() and np.array_equal(got["match_out"], row)
            continue
        c12, c21 = ap.sim3_hops(pr["s12"], pr["R12"], pr["t12"])
        m1, m2 = got["matched"]
        queries = []
        for d, (kf, cam, hop, matched) in enumerate(((kf1, sc["cameras"][a], c21, m1), (kf2, sc["cameras"][b], c12, m2))):
            pts = kf["points"]
            ok = ((pts["flags"] & ss.lr.SKIP) == 0) & ~matched
            with np.errstate(all="ignore"):
                q = ap.sim3_direction(hb, cam_ns(sc["cameras"][a]), cam_ns(sc["cameras"][a]), T_of(cam), hop, pts["pos"], pts["min_distance"],
                                      pts["max_distance"], pts["desc"], np.arange(len(pts)), ok, sf[1], len(sf))
            seen = np.nonzero(got["reason"][d] >= R["empty"])[0]
            assert np.array_equal(q["src"], seen), (p, d)
            assert np.array_equal(q["u"], got["u"][d][seen]) and np.array_equal(q["v"], got["v"][d][seen]), (p, d)
            assert np.array_equal(q["level"], got["level"][d][seen]), (p, d, "the table form and the logf form of PredictScale differ: move the point")
            queries.append(q)
        v1, keep1 = hb.frame_view(kf1["kps"], kf1["desc"], None, bounds)
        v2, keep2 = hb.frame_view(kf2["kps"], kf2["desc"], None, bounds)
        found, m12 = hb.search_sim3("oracle", v1, v2, queries[0], queries[1], sf, sf, float(pr["th"]))
        print(f"pair {p} {sc['names'][p]}: found {got['stats']['n_found']} / {found}")
        assert found == got["stats"]["n_found"], p
        assert np.array_equal(np.where(m12 >= 0, m12, row), got["match_out"]), p
        assert ((m12 < 0) | (row == -1)).all(), p


def test_host_compilation_of_the_core_equals_the_restatement(shared):
    sc, results = shared
    for p, got in enumerate(results):
        a, b = int(sc["slots1"][p]), int(sc["slots2"][p])
        pr = sc["pairs"][p]
        for d, f in enumerate((a, b)):
            kf = ss.keyframe(sc, f)
            u, v, level, reason = hsb.project(sc["cameras"][f], sc["cameras"][a], pr["R12"], pr["t12"], pr["s12"], d, kf["points"], got["matched"][d],
                                              sc["sf"], sc["bounds"])
            want = np.where(got["reason"][d] >= R["empty"], 0, got["reason"][d])
            assert np.array_equal(reason, want), (p, d)
            assert u.tobytes() == got["u"][d].tobytes() and v.tobytes() == got["v"][d].tobytes() and np.array_equal(level, got["level"][d]), (p, d)


def test_scene_holds_the_cases(shared):
    sc, results = shared
    names, cap = sc["names"], sc["capacity"]
    pair = {n: p for p, n in enumerate(names)}
    sizes = sorted(int(c) for c in sc["counts"])
    assert all(k in sizes for k in (0, 37, 300, 600, 31, 33, 257)) and max(sizes) < cap and cap % 32 != 0
    slots = list(zip(sc["slots1"].tolist(), sc["slots2"].tolist()))
    assert sc["counts"][slots[pair["empty_1"]][0]] == 0 and sc["counts"][slots[pair["empty_2"]][1]] == 0
    assert slots[pair["same"]][0] == slots[pair["same"]][1]
    assert slots[pair["truth"]] == slots[pair["other_sim3"]] and not np.array_equal(sc["pairs"][pair["truth"]]["R12"], sc["pairs"][pair["other_sim3"]]["R12"])
    assert len({s[0] for s in slots}) < len(slots)  # pairs share keyframe 1's slot, as LoopClosing's candidates do
    assert {float(x) for x in sc["pairs"]["s12"]} >= {0.5, 1.0, 2.0}
    st = results[pair["behind"]]["stats"]
    assert st["n_in_view_12"] == 0 and (results[pair["behind"]]["reason"][0] == R["behind"]).sum() > 100
    for d in (0, 1):  # every exit in both directions
        seen = np.concatenate([r["reason"][d] for r in results])
        for name, code in R.items():
            assert (seen == code).sum() >= 1, (d, name)
    # the hand points of the pair (2, 2): on the bounds, on the band's edges, at the threshold, a tie
    h, r = sc["hand"], results[pair["same"]]
    why, u, m1 = r["reason"][0], r["u"][0], r["match1"]
    assert why[h["u_min"]] >= R["empty"] and u[h["u_min"]] == f32(ss.BOUNDS[0])
    pts = sc["points"][2]
    assert why[h["u_max"]] == R["image"] and f32(f32(512) * f32(pts["pos"][h["u_max"]][0] * f32(0.5))) + f32(320) == f32(ss.BOUNDS[1])
    assert why[h["band_lo_in"]] >= R["empty"] and why[h["band_lo_out"]] == R["near"]
    assert why[h["band_hi_in"]] >= R["empty"] and why[h["band_hi_out"]] == R["far"]
    assert why[h["behind"]] == R["behind"] and why[h["z_zero"]] == R["image"]
    infos = {i["feature"]: i for i in r["infos"][0]}
    assert m1[h["dist_100"]] == h["target_dist_100"] and infos[h["dist_100"]]["best"] == 100
    assert m1[h["dist_101"]] == -1 and why[h["dist_101"]] == R["none"] and infos[h["dist_101"]]["best"] == 101
    assert infos[h["tie"]]["tie"] and m1[h["tie"]] == h["target_tie_b"] > h["target_tie"]  # the earlier CSR position: the LATER feature
    # windows: clipped at each border, wider than eight grid columns, a single cell
    every = [i for r in results for d in (0, 1) for i in r["infos"][d]]
    assert any(i["u"] - i["r"] < ss.BOUNDS[0] for i in every) and any(i["u"] + i["r"] > ss.BOUNDS[1] for i in every)
    assert any(i["v"] - i["r"] < ss.BOUNDS[2] for i in every) and any(i["v"] + i["r"] > ss.BOUNDS[3] for i in every)
    assert max(i["columns"] for i in every) > 8 and min(i["cells"] for i in every if i["cells"]) == 1
    levels = np.concatenate([r["level"][d][r["reason"][d] >= R["empty"]] for r in results for d in (0, 1)])
    assert (levels == 0).any() and (levels == len(sc["sf"]) - 1).any()
    # the rows
    kinds = np.zeros(4, int)
    for p, (a, b) in enumerate(slots):
        n1, n2 = int(sc["counts"][a]), int(sc["counts"][b])
        row = sc["rows"][p][:n1]
        kinds += [(row == -1).sum(), ((row >= 0) & (row < n2)).sum(), (row == ss.MATCHED_ELSEWHERE).sum(), (row >= n2).sum()]
        assert (sc["rows"][p][n1:] == ss.POISON).all()
    assert (kinds > 0).all(), kinds
    # a keyframe-2 feature kept out of direction 2 only because a row entry marks it: without the mark its window is searched
    a, b = slots[pair["truth"]]
    r = results[pair["truth"]]
    marked = np.nonzero(r["reason"][1] == R["matched"])[0]
    h12, _ = ss.hops(*(sc["pairs"][pair["truth"]][k] for k in ("R12", "t12", "s12")))
    assert any(ss.project(sc["cameras"][b], h12, sc["cameras"][a], sc["points"][b][i], sc["sf"], sc["bounds"])[0] == 0 for i in marked)
    # what the agreement pass is for
    doubled = 0
    for p, r in enumerate(results):
        s = r["stats"]
        if names[p] not in sc["degenerate"]:
            assert s["n_found"] >= 10 and s["n_single_12"] - s["n_found"] >= 3 and s["n_single_21"] - s["n_found"] >= 3, (names[p], s)
        m1 = r["match1"]
        for j in np.unique(m1[m1 >= 0]):
            who = np.nonzero(m1 == j)[0]
            doubled += len(who) > 1 and r["match2"][j] in who
    assert doubled >= 1


def struct_bytes(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n = 0
    for kind, decl in re.findall(r"(float|int32_t) ([^;]+);", body):
        for field in decl.split(","):
            m = re.search(r"\[(\d+)\]", field)
            n += int(m.group(1)) if m else 1
    return 4 * n


def test_exports_and_struct_sizes(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    for name in ("amos_match_sim3_search_batch_device", "amos_match_sim3_search"):
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "amos_frontend.h")).read()
    source = open(os.path.join(ROOT, "amos-slam_amd", "csrc", "amos_sim3_search.hip")).read()
    pair, stats = struct_bytes(header, "amos_sim3_search_pair"), struct_bytes(header, "amos_sim3_search_stats")
    assert pair == pkg.SIM3_SEARCH_PAIR_DTYPE.itemsize == ss.PAIR.itemsize and f"sizeof(amos_sim3_search_pair) == {pair}" in source
    assert stats == pkg.SIM3_SEARCH_STATS_DTYPE.itemsize == 4 * len(ss.STATS) and f"sizeof(amos_sim3_search_stats) == {stats}" in source
    assert pkg.SIM3_SEARCH_STATS_DTYPE.names == ss.STATS
    assert "#define AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE (-2)" in header and pkg.SIM3_SEARCH_MATCHED_ELSEWHERE == ss.MATCHED_ELSEWHERE == -2
    n_ptr = len(re.findall(r"\*", re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct amos_sim3_search \{(.*?)\} amos_sim3_search;", header, re.S).group(1), flags=re.S)))
    assert C.sizeof(pkg.Sim3Search) == 8 * n_ptr + 4 * 8


def test_the_c_entries_reject_bad_arguments_without_a_device(pkg):
    """validation comes before the device (and before the handle is looked into: a zeroed buffer stands in for it)"""
    L = pkg.lib()
    fake = C.create_string_buffer(4096)
    buf = np.zeros(1 << 16, np.uint8)
    cams = np.zeros(2, pkg.SIM3_CAMERA_DTYPE)
    cams["fx"] = cams["fy"] = 500.0
    sf = ss.SCALE
    keep = []

    def pairs_of(**kw):
        pr = np.array([pkg.sim3_search_pair(np.eye(3), [0.1, 0, 0], 1.0)] * 2)
        for k, v in kw.items():
            pr[k][1] = v
        return pr

    def struct_of(**kw):
        pr, cam = kw.pop("pairs", pairs_of()), kw.pop("cameras", cams)
        keep.extend([pr, cam])
        p = buf.ctypes.data
        d = dict(d_kps=p, d_desc=p, d_counts=p, d_cell_start=p, d_items=p, d_points=p, cameras=None if cam is None else cam.ctypes.data,
                 scale_factors=sf.ctypes.data, d_pairs_1=p, d_pairs_2=p, pairs=None if pr is None else pr.ctypes.data, d_sim3=None, d_match12=p,
                 d_match_out=p, d_match1=p + 4096, d_match2=p + 8192, d_stats=p, n_frames=2, n_pairs=2, capacity=64, n_levels=8, min_x=0.0, max_x=640.0,
                 min_y=0.0, max_y=480.0)
        d.update(kw)
        return pkg.Sim3Search(**d)

    bad_cam = cams.copy()
    bad_cam["tcw"][1, 2] = np.nan
    nan_R = np.eye(3)
    nan_R[1, 1] = np.nan
    p = buf.ctypes.data
    bad = [struct_of(**{k: None}) for k in ("d_kps", "d_desc", "d_counts", "d_cell_start", "d_items", "d_points", "cameras", "scale_factors", "d_pairs_1",
                                            "d_pairs_2", "pairs", "d_match12", "d_match_out", "d_match1", "d_match2", "d_stats")]
    bad += [struct_of(n_pairs=0), struct_of(n_frames=0), struct_of(capacity=0), struct_of(capacity=65537), struct_of(n_levels=0),
            struct_of(n_levels=MAX_LEVELS + 1), struct_of(max_x=0.0), struct_of(max_y=0.0), struct_of(min_x=np.nan), struct_of(cameras=bad_cam),
            struct_of(pairs=pairs_of(R12=nan_R.reshape(9))), struct_of(pairs=pairs_of(t12=[0, np.inf, 0])), struct_of(pairs=pairs_of(s12=0.0)),
            struct_of(pairs=pairs_of(s12=-1.0)), struct_of(pairs=pairs_of(s12=np.nan)), struct_of(pairs=pairs_of(th=0.0)),
            struct_of(pairs=pairs_of(th=np.nan)), struct_of(pairs=pairs_of(th=np.inf)), struct_of(d_match1=p), struct_of(d_match2=p),
            struct_of(d_match_out=p + 4096), struct_of(d_match_out=p + 8192), struct_of(d_match2=p + 4096),
            struct_of(d_sim3=p, pairs=pairs_of(th=-1.0))]
    for k, s in enumerate(bad):
        assert L.amos_match_sim3_search_batch_device(fake, C.byref(s)) == ERR_INVALID, k
    assert L.amos_match_sim3_search_batch_device(None, C.byref(struct_of())) == ERR_INVALID
    assert L.amos_match_sim3_search_batch_device(fake, None) == ERR_INVALID
    # the host form
    kps, desc, pts = np.zeros(4, pkg.KP_DTYPE), np.zeros((4, 32), np.uint8), np.zeros(4, pkg.MAP_POINT_DTYPE)
    row, out, stats = np.full(4, -1, np.int32), np.zeros(4, np.int32), np.zeros(1, pkg.SIM3_SEARCH_STATS_DTYPE)

    def view(n=4, keys=kps, d=desc, bounds=(0.0, 640.0, 0.0, 480.0)):
        v = pkg.FrameView()
        v.n, v.keys_un, v.descriptors, v.u_right = n, None if keys is None else keys.ctypes.data, None if d is None else d.ctypes.data, None
        v.min_x, v.max_x, v.min_y, v.max_y = bounds
        keep.append(v)
        return C.addressof(v)

    def host(**kw):
        a = dict(m=fake, kf1=view(), points1=pts, kf2=view(), points2=pts, cameras=cams, sim3=pairs_of()[:1], sf=sf, n_levels=8, match12=row,
                 match_out=out, match1=None, match2=None, stats=stats)
        a.update(kw)
        keep.append(a)
        args = [x.ctypes.data if isinstance(x, np.ndarray) else x for x in a.values()]
        return L.amos_match_sim3_search(*args)

    def one(**kw):
        pr = np.array([pkg.sim3_search_pair(np.eye(3), [0.1, 0, 0], 1.0)])
        for k, v in kw.items():
            pr[k][0] = v
        return pr

    for kw in (dict(m=None), dict(kf1=None), dict(kf2=None), dict(points1=None), dict(points2=None), dict(cameras=None), dict(sim3=None), dict(sf=None),
               dict(match12=None), dict(match_out=None), dict(stats=None), dict(n_levels=0), dict(n_levels=MAX_LEVELS + 1), dict(kf1=view(n=-1)),
               dict(kf2=view(n=65537)), dict(kf1=view(keys=None)), dict(kf2=view(d=None)), dict(kf2=view(bounds=(0.0, 641.0, 0.0, 480.0))),
               dict(kf1=view(bounds=(0.0, 0.0, 0.0, 480.0)), kf2=view(bounds=(0.0, 0.0, 0.0, 480.0))), dict(cameras=bad_cam), dict(sim3=one(s12=0.0)),
               dict(sim3=one(th=0.0)), dict(sim3=one(t12=[np.nan, 0, 0]))):
        assert host(**kw) == ERR_INVALID, kw


def case_file(path, cam_from, cam1, pr, direction, points, sf, bounds):
    with open(path, "wb") as f:
        f.write(np.array([len(points), len(sf), direction, 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(cam_from, ss.CAMERA).tobytes() + np.ascontiguousarray(cam1, ss.CAMERA).tobytes())
        f.write(pr["R12"].astype(f32).tobytes() + pr["t12"].astype(f32).tobytes() + f32(pr["s12"]).tobytes())
        f.write(np.asarray(bounds, f32).tobytes() + np.asarray(sf, f32).tobytes() + np.ascontiguousarray(points, ss.MAP_POINT).tobytes())


def test_the_core_as_a_sanitized_plain_program_equals_the_restatement(shared, tmp_path):
    """Host code in a stand-alone program with its own main, compiled with -fsanitize=address,undefined: it must end clean with the
    restatement's projections (u and v compared as bit patterns) for a few hundred points per direction, the hand points among them."""
    sc, results = shared
    exe = str(tmp_path / "sim3_search_core_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "host_sim3_search", "sim3_search_core_main.cc")], check=True)
    cases, paths = [], []
    for name in ("same", "half", "double", "behind"):
        p = sc["names"].index(name)
        a, b = int(sc["slots1"][p]), int(sc["slots2"][p])
        for d, f in enumerate((a, b)):
            paths.append(str(tmp_path / f"{name}_{d}.bin"))
            case_file(paths[-1], sc["cameras"][f], sc["cameras"][a], sc["pairs"][p], d, ss.keyframe(sc, f)["points"], sc["sf"], sc["bounds"])
            cases.append((p, d, f))
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    blocks = run.stdout.split("case ")[1:]
    assert len(blocks) == len(cases)
    for (p, d, f), block in zip(cases, blocks):
        got = np.array([[int(x) for x in line.split()] for line in block.strip().split("\n")[1:]], np.int64)
        pts = ss.keyframe(sc, f)["points"]
        cam_from, cam1, pr = sc["cameras"][f], sc["cameras"][int(sc["slots1"][p])], sc["pairs"][p]
        h12, h21 = ss.hops(pr["R12"], pr["t12"], pr["s12"])
        assert len(got) == len(pts) > 200
        for i, point in enumerate(pts):  # (the program knows no row: every point is projected)
            if point["flags"] & ss.lr.SKIP:
                want = (R["no_point"], 0, f32(0), f32(0))
            else:
                want = ss.project(cam_from, h21 if d == 0 else h12, cam1, point, sc["sf"], sc["bounds"])
                want = (want[0], want[3], want[1], want[2])
            assert tuple(got[i]) == (i, want[0], want[1], int(f32(want[2]).view(np.uint32)), int(f32(want[3]).view(np.uint32))), (p, d, i)
