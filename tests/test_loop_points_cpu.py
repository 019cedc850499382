"""CPU: the loop-closing point search without a GPU.  The restatement of ORBmatcher::SearchByProjection(pKF, Scw, ...)
(tests/loop_points_restatement.py) must equal the pre-filter of tests/adaptor_prefilter.py fed to the oracle's view-based search on both
queries of the scene the GPU tests use; the host compilation of amos-slam_amd/csrc/amos_loop_points_core.h must equal
adaptor_prefilter.unscaled / centre bit for bit; that scene must hold every case the GPU tests rely on -- so a pass on the GPU means
something; the exports, the struct sizes and the C entries' argument checks; the core as a stand-alone program under
-fsanitize=address,undefined."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import adaptor_prefilter as ap
import host_binding as hb
import host_loop_points_binding as hlb
import local_points_restatement as lr
import loop_points_restatement as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ERR_INVALID, MAX_LEVELS = -1, 16  # AMOS_ERR_INVALID, AMOS_MAX_LEVELS (include/amos_frontend.h)
R = lp.REASONS


@pytest.fixture(scope="module")
def shared():
    return lp.shared()


def scw_samples():
    """the scene's two, the hand case's, and seeded ones with scales from 1e-3 to 1e3"""
    sc, _ = lp.shared()
    rng = np.random.default_rng(3)
    out = [q["Scw"].reshape(4, 4) for q in sc["queries"]] + [lp.hand_greedy()["query"]["Scw"].reshape(4, 4)]
    for _ in range(200):
        out.append(lp.scw_of(10.0 ** rng.uniform(-3, 3), *rng.uniform(-3, 3, 3), rng.uniform(-5, 5, 3)))
    return out


def test_restatement_equals_prefilter_plus_oracle(ob, shared):
    """The queries from adaptor_prefilter.keyframe_queries (with the level in its table form), the greedy search from the oracle's
    orc_window_search with the entry row as its occupied array, at th 10."""
    sc, results = shared
    sf, bounds = sc["sf"], sc["bounds"]
    shim = types.SimpleNamespace(WINDOW_QUERY=hb.WINDOW_QUERY,
                                 standin_predict_scale=lambda md, cd, _sf1, _nl: lr.table_level(np.asarray(md, f32) / np.asarray(cd, f32), sf))
    for k, got in enumerate(results):
        q = sc["queries"][k]
        kps, desc = sc["kfs"][int(q["frame"])]
        a, c = int(sc["first"][k]), int(sc["count"][k])
        pts = sc["points"][a:a + c]
        fd = lp.found_of(len(kps), c, q, sc["rows"][k], sc["found"][a:a + c], sc["maps"][k])
        Rcw, tcw = ap.unscaled(q["Scw"].reshape(4, 4))
        cam = types.SimpleNamespace(fx=q["fx"], fy=q["fy"], cx=q["cx"], cy=q["cy"], mbf=0.0, min_x=bounds[0], max_x=bounds[1], min_y=bounds[2],
                                    max_y=bounds[3])
        keep = ((pts["flags"] & lp.SKIP) == 0) & ~fd
        with np.errstate(all="ignore"):
            wq, pos = ap.keyframe_queries(shim, cam, Rcw, tcw, ap.centre(Rcw, tcw), pts["pos"], pts["normal"], pts["min_distance"], pts["max_distance"],
                                          pts["desc"], np.arange(c), keep, False, sf[1], len(sf))
        assert np.array_equal(pos, np.nonzero(got["in_view"])[0]), k
        assert wq["u"].tobytes() == got["u"][pos].tobytes() and wq["v"].tobytes() == got["v"][pos].tobytes(), k
        assert np.array_equal(wq["level"], got["level"][pos]), k
        view, keepalive = hb.frame_view(kps, desc, None, tuple(float(b) for b in bounds))
        n, m = hb.search_projection_sim("oracle", view, wq, sc["rows"][k], sf, 10)
        new = (sc["rows"][k] == -1) & (m != -1)
        want = np.where(new, pos[np.clip(m, 0, max(len(pos) - 1, 0))], -1)
        print(f"query {k}: {got['n_matches']} / {n} matches")
        assert n == got["n_matches"] == int(new.sum()), k
        assert np.array_equal(want, got["loop_match"]), k
        assert np.array_equal(m[~new], sc["rows"][k][~new]), k


def test_host_compilation_of_the_core_equals_the_adaptor_prefilter():
    for S in scw_samples():
        Rw, tw = ap.unscaled(S)
        Ow = ap.centre(Rw, tw)
        r0 = S[0, :3].astype(np.float64)
        scw = f32(np.sqrt(r0[0] * r0[0] + r0[1] * r0[1] + r0[2] * r0[2]))
        Rg, tg, Og, sg = hlb.unscale(S)
        assert Rg.tobytes() == Rw.astype(f32).tobytes() and tg.tobytes() == tw.astype(f32).tobytes() and Og.tobytes() == Ow.tobytes()
        assert f32(sg).tobytes() == scw.tobytes()


def test_scene_holds_the_cases(shared):
    sc, results = shared
    a, b = results
    assert 280 <= len(sc["kfs"][0][0]) <= 360 and 280 <= len(sc["kfs"][1][0]) <= 360 and sc["count"][0] == 600
    for q in sc["queries"]:  # a Sim3 with a scale other than 1
        assert abs(float(lp.f64(np.linalg.norm(q["Scw"][:3].astype(np.float64)))) - 1.0) > 0.05
    # every pre-filter step rejects a point; bad, d_found and the feature map each skip one
    for name in ("bad", "found", "behind", "image", "near", "far", "angle"):
        assert (a["reason"] == R[name]).sum() >= 1, name
    q0 = sc["queries"][0]
    n0, c0 = len(sc["kfs"][0][0]), int(sc["count"][0])
    by_bytes = lp.found_of(n0, c0, lp.query(0, q0["Scw"]), sc["rows"][0], sc["found"][:c0], None)
    by_map = lp.found_of(n0, c0, q0, sc["rows"][0], None, sc["maps"][0])
    good = (sc["points"][:c0]["flags"] & lp.SKIP) == 0
    assert (by_bytes & good).sum() >= 1 and (by_map & good & ~by_bytes).sum() >= 1 and int(q0["found_from_match"]) == 1
    assert (sc["rows"][0] == lp.MATCHED_ELSEWHERE).sum() >= 1 and (sc["rows"][0] >= 0).sum() >= 1
    infos = a["infos"].values()
    assert sum(i["occupied_on_entry"] > 0 for i in infos) >= 10          # features occupied on entry inside searched windows
    assert sum(i["best_taken"] and i["second_free"] for i in infos) >= 10  # the second of the entry record is taken
    assert sum(i["both_taken"] for i in infos) >= 3 and sum(i["researched"] for i in infos) == a["n_researched"] >= 3  # the research path
    assert sum(i["researched"] and i["accepted"] for i in infos) >= 1     # ... and it finds a third feature
    far = [i for i in infos if i["best_taken"] and len(i["entry"]) == 2 and i["entry"][1][0] > 50]  # the best taken, the second beyond max_dist
    assert sum(i["second_free"] for i in far) >= 1 and sum(i["both_taken"] and not i["researched"] for i in far) >= 1 and not any(i["accepted"] for i in far)
    assert sum(i["only_taken"] for i in infos) >= 1                       # the only candidate is taken
    for p in sc["only_points"][1:]:
        assert a["infos"][p]["only_taken"] and not a["infos"][p]["accepted"]
    t50, t51 = sc["th_points"]
    assert a["infos"][t50]["best_free"] == 50 and a["infos"][t50]["accepted"] and a["infos"][t51]["best_free"] == 51 and not a["infos"][t51]["accepted"]
    assert (a["loop_match"] == t50).sum() == 1 and (a["loop_match"] == t51).sum() == 0
    # n_total on both sides of min_total
    assert a["n_total"] >= 40 and a["accepted"] == 1 and 0 < b["n_total"] < 40 and b["accepted"] == 0 and b["n_matches"] > 10
    assert sc["capacity"] > max(n0, len(sc["kfs"][1][0])) and sc["capacity"] % 32 != 0
    # the hand case: the third point's answer depends on the first two accepts
    h = lp.hand_greedy()
    free = np.full(2, -1, np.int32)
    r = lp.search(h["kps"], h["desc"], h["points"], h["query"], free, None, None, lp.SCALE, lp.BOUNDS)
    assert np.array_equal(r["loop_match"], h["expected"]) and r["n_matches"] == 2 and r["n_researched"] == 1
    alone = lp.search(h["kps"], h["desc"], h["points"][2:], h["query"], free, None, None, lp.SCALE, lp.BOUNDS)
    assert np.array_equal(alone["loop_match"], [-1, 0])


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
    for name in ("amos_match_loop_points_batch_device", "amos_match_loop_points"):
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "amos_frontend.h")).read()
    source = open(os.path.join(ROOT, "amos-slam_amd", "csrc", "amos_loop_points.hip")).read()
    query, stats = struct_bytes(header, "amos_loop_points_query"), struct_bytes(header, "amos_loop_points_stats")
    assert query == pkg.LOOP_POINTS_QUERY_DTYPE.itemsize == lp.QUERY.itemsize and f"sizeof(amos_loop_points_query) == {query}" in source
    assert stats == pkg.LOOP_POINTS_STATS_DTYPE.itemsize == 4 * len(lp.STATS) and f"sizeof(amos_loop_points_stats) == {stats}" in source
    assert pkg.LOOP_POINTS_STATS_DTYPE.names == lp.STATS and pkg.LOOP_POINTS_QUERY_DTYPE.names == lp.QUERY.names
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct amos_loop_points_search \{(.*?)\} amos_loop_points_search;", header, re.S).group(1), flags=re.S)
    assert C.sizeof(pkg.LoopPointsSearch) == 8 * len(re.findall(r"\*", body)) + 4 * 9 + 4  # (the struct's size is a multiple of 8)


def test_the_c_entries_reject_bad_arguments_without_a_device(pkg):
    """validation comes before the device (and before the handle is looked into: a zeroed buffer stands in for it)"""
    L = pkg.lib()
    fake = C.create_string_buffer(4096)
    buf = np.zeros(1 << 16, np.uint8)
    sf = lp.SCALE
    keep = []
    S = lp.scw_of(0.9, 0.01, 0.02, 0.03, [0.1, 0.2, 0.3])

    def queries_of(**kw):
        qs = np.array([lp.query(0, S), lp.query(1, S)], lp.QUERY)
        for k, v in kw.items():
            qs[k][1] = v
        return qs

    first, count = np.array([0, 10], np.int32), np.array([10, 20], np.int32)

    def struct_of(**kw):
        qs = kw.pop("queries", queries_of())
        p0, pc = kw.pop("point_first", first), kw.pop("point_count", count)
        keep.extend([qs, p0, pc])
        p = buf.ctypes.data
        d = dict(d_kps=p, d_desc=p, d_counts=p, d_cell_start=p, d_items=p, scale_factors=sf.ctypes.data, d_points=p,
                 point_first=None if p0 is None else p0.ctypes.data, point_count=None if pc is None else pc.ctypes.data,
                 queries=None if qs is None else qs.ctypes.data, d_opt=None, d_matched=p, d_found=None, d_point_of_feature2=None, d_loop_match=p + 8192,
                 d_stats=p + 4096, n_frames=2, n_queries=2, n_points=30, capacity=64, n_levels=8, min_x=0.0, max_x=640.0, min_y=0.0, max_y=480.0)
        d.update(kw)
        return pkg.LoopPointsSearch(**d)

    def scw(r, c, v):
        T = S.copy()
        T[r, c] = v
        return T.reshape(16)

    zero_row = S.copy()
    zero_row[0, :3] = 0
    bad = [struct_of(**{k: None}) for k in ("d_kps", "d_desc", "d_counts", "d_cell_start", "d_items", "scale_factors", "d_points", "point_first",
                                            "point_count", "queries", "d_matched", "d_loop_match", "d_stats")]
    bad += [struct_of(n_queries=0), struct_of(n_frames=0), struct_of(n_points=-1), struct_of(capacity=0), struct_of(capacity=65537),
            struct_of(n_levels=0), struct_of(n_levels=MAX_LEVELS + 1), struct_of(max_x=0.0), struct_of(max_y=0.0), struct_of(min_x=np.nan),
            struct_of(queries=queries_of(frame=2)), struct_of(queries=queries_of(frame=-1)),
            struct_of(point_first=np.array([0, -1], np.int32)), struct_of(point_count=np.array([10, 21], np.int32)),
            struct_of(point_count=np.array([10, -1], np.int32)), struct_of(point_first=np.array([0, 31], np.int32)),
            struct_of(queries=queries_of(th=np.nan)), struct_of(queries=queries_of(th=np.inf)), struct_of(queries=queries_of(th=0.0)),
            struct_of(queries=queries_of(fx=np.nan)), struct_of(queries=queries_of(cy=np.inf)),
            struct_of(queries=queries_of(Scw=scw(1, 1, np.nan))), struct_of(queries=queries_of(Scw=scw(2, 3, np.inf))),
            struct_of(queries=queries_of(Scw=zero_row.reshape(16))),
            struct_of(queries=queries_of(max_dist=-1)), struct_of(queries=queries_of(max_dist=256)),
            struct_of(queries=queries_of(enabled=2)), struct_of(queries=queries_of(enabled=-1)), struct_of(queries=queries_of(found_from_match=2)),
            struct_of(queries=queries_of(found_from_match=1)),  # without d_point_of_feature2
            struct_of(d_opt=buf.ctypes.data, queries=queries_of(th=-1.0))]
    for k, s in enumerate(bad):
        assert L.amos_match_loop_points_batch_device(fake, C.byref(s)) == ERR_INVALID, k
        assert b"amos_match_loop_points_batch_device" in pkg.lib().amos_last_error(), k
    assert L.amos_match_loop_points_batch_device(None, C.byref(struct_of())) == ERR_INVALID
    assert L.amos_match_loop_points_batch_device(fake, None) == ERR_INVALID
    # the host form
    kps, desc, pts = np.zeros(4, pkg.KP_DTYPE), np.zeros((4, 32), np.uint8), np.zeros(6, pkg.MAP_POINT_DTYPE)
    row, out, stats = np.full(4, -1, np.int32), np.zeros(4, np.int32), np.zeros(1, pkg.LOOP_POINTS_STATS_DTYPE)
    pf2 = np.full(5, -1, np.int32)

    def view(n=4, keys=kps, d=desc, bounds=(0.0, 640.0, 0.0, 480.0)):
        v = pkg.FrameView()
        v.n, v.keys_un, v.descriptors, v.u_right = n, None if keys is None else keys.ctypes.data, None if d is None else d.ctypes.data, None
        v.min_x, v.max_x, v.min_y, v.max_y = bounds
        keep.append(v)
        return C.addressof(v)

    def one(**kw):
        q = np.array([lp.query(0, S)], lp.QUERY)
        for k, v in kw.items():
            q[k][0] = v
        return q

    def host(**kw):
        a = dict(m=fake, kf=view(), points=pts, n_points=6, query=one(), matched=row, found=None, pf2=None, n2=0, sf=sf, n_levels=8, loop_match=out,
                 stats=stats)
        a.update(kw)
        keep.append(a)
        args = [x.ctypes.data if isinstance(x, np.ndarray) else x for x in a.values()]
        return L.amos_match_loop_points(*args)

    for kw in (dict(m=None), dict(kf=None), dict(points=None), dict(n_points=-1), dict(query=None), dict(sf=None), dict(loop_match=None),
               dict(stats=None), dict(n_levels=0), dict(n_levels=MAX_LEVELS + 1), dict(kf=view(n=-1)), dict(kf=view(n=65537)), dict(kf=view(keys=None)),
               dict(kf=view(d=None)), dict(kf=view(bounds=(0.0, 0.0, 0.0, 480.0))), dict(n2=5), dict(n2=-1), dict(pf2=pf2, n2=65537),
               dict(query=one(frame=1)), dict(query=one(th=0.0)), dict(query=one(Scw=zero_row.reshape(16))), dict(query=one(max_dist=300)),
               dict(query=one(enabled=3)), dict(query=one(found_from_match=1)), dict(query=one(fx=np.nan))):
        assert host(**kw) == ERR_INVALID, kw


def test_the_core_as_a_sanitized_plain_program_equals_the_adaptor_prefilter(tmp_path):
    """Host code in a stand-alone program with its own main, compiled with -fsanitize=address,undefined: it must end clean with
    adaptor_prefilter's decomposition (compared as bit patterns) for a few hundred Scw."""
    exe = str(tmp_path / "loop_points_core_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "host_loop_points", "loop_points_core_main.cc")], check=True)
    samples = scw_samples()
    path = str(tmp_path / "scw.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(samples)], np.int32).tobytes() + np.array(samples, f32).tobytes())
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    lines = run.stdout.strip().split("\n")[1:]
    assert len(lines) == len(samples) > 200
    for i, (S, line) in enumerate(zip(samples, lines)):
        got = np.array([int(x) for x in line.split()], np.int64)
        Rw, tw = ap.unscaled(S)
        r0 = S[0, :3].astype(np.float64)
        scw = f32(np.sqrt(r0[0] * r0[0] + r0[1] * r0[1] + r0[2] * r0[2]))
        want = np.concatenate([Rw.astype(f32).reshape(9), tw.astype(f32), ap.centre(Rw, tw), [scw]]).astype(f32).view(np.uint32)
        assert got[0] == i and np.array_equal(got[1:], want.astype(np.int64)), i
