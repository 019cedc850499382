"""amos_match_new_points_batch_device on the GPU against tests/new_points_restatement.py, bit for bit: d_new up to n_new with the poison
behind it preserved, d_verdict over the whole row, d_stats.  The restatement is held to the host compilation of the core header, to an
independent SVD and to its cases' own checks in test_new_points_cpu.py."""
import numpy as np
import pytest

import host_new_points_binding as hnb
import kf_search_cases as kc
import new_points_cases as nc
import new_points_restatement as nr

pytestmark = pytest.mark.gpu


def _up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def outputs(n_pairs, cap):
    """device buffers with poison that the call must overwrite (verdict, stats) or preserve beyond n_new (new)"""
    import torch
    d_new = _up(np.full((n_pairs, cap), np.array(hnb.POISON_NEW, nr.NEW_POINT), nr.NEW_POINT))
    d_verdict = torch.full((n_pairs, cap), 77, dtype=torch.int32, device="cuda")
    d_stats = torch.full((n_pairs, 16), -9, dtype=torch.int32, device="cuda")
    return d_new, d_verdict, d_stats


def fetch(d_new, d_verdict, d_stats, n_pairs, cap):
    new = np.frombuffer(d_new.cpu().numpy().tobytes(), nr.NEW_POINT).reshape(n_pairs, cap)
    stats = np.frombuffer(d_stats.cpu().numpy().tobytes(), nr.NEW_POINTS_STATS)
    return new, None if d_verdict is None else d_verdict.cpu().numpy(), stats


def run_device(pkg, case, pad=5, with_verdict=True, with_raw=True, with_right=True, mt=None):
    import torch
    a = hnb.pack(case, pad, with_raw, with_right)
    cap, n_pairs = a["capacity"], len(a["pairs"])
    d = {k: None if a[k] is None else _up(a[k]) for k in ("kps", "kps_raw", "counts", "u_right", "depth", "match", "scale", "sigma2")}
    d_1, d_2 = _up(np.ascontiguousarray(a["pairs"][:, 0])), _up(np.ascontiguousarray(a["pairs"][:, 1]))
    d_new, d_verdict, d_stats = outputs(n_pairs, cap)
    if not with_verdict:
        d_verdict = None
    torch.cuda.synchronize()
    own = mt is None
    mt = mt or pkg.OrbMatcher()
    mt.new_points_batch_device(d["kps"].data_ptr(), d["counts"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(), a["pairs"], cap, d["match"].data_ptr(),
                               d["scale"].data_ptr(), d["sigma2"].data_ptr(), len(a["scale"]), a["cams"], d_new.data_ptr(), d_stats.data_ptr(),
                               d_verdict=_ptr(d_verdict), d_u_right=_ptr(d["u_right"]), d_depth=_ptr(d["depth"]), d_kps_raw=_ptr(d["kps_raw"]),
                               enabled=a["enabled"])
    mt.sync()
    out = fetch(d_new, d_verdict, d_stats, n_pairs, cap)
    if own:
        mt.close()
    return out, cap


def check(pkg, case, **kw):
    (new, verdict, stats), cap = run_device(pkg, case, **kw)
    want_new, want_verdict, want_stats = hnb.expected(hnb.stripped(case, kw.get("with_raw", True), kw.get("with_right", True)), cap)
    for p in range(len(stats)):
        print(f"pair {p}: n_matches {stats['n_matches'][p]} n_new {stats['n_new'][p]} verdicts {stats['n_verdict'][p].tolist()} status "
              f"{stats['status'][p]} / restatement {want_stats['n_verdict'][p].tolist()}")
    assert stats.tobytes() == want_stats.tobytes()
    if verdict is not None:
        assert verdict.tobytes() == want_verdict.tobytes()
    assert new.tobytes() == want_new.tobytes()  # (the poison beyond n_new included)
    return want_stats


@pytest.mark.parametrize("name", sorted(nc.hand_cases()))
def test_hand_cases(gpu_lib, name):
    case = nc.hand_cases()[name]
    assert max(len(s["keys"]) for s in case["sides"]) <= 2
    check(gpu_lib, case, pad=nc.CAPACITY - max(len(s["keys"]) for s in case["sides"]))  # capacity 8


@pytest.mark.parametrize("name", sorted(nc.random_cases()))
def test_random_pairs(gpu_lib, name):
    stats = check(gpu_lib, nc.random_cases()[name])
    assert stats["n_new"].sum() > 0 and stats["n_verdict"][1, nr.CLAIMED] > 0


@pytest.mark.parametrize("n", nc.COUNTS)
def test_feature_counts(gpu_lib, n):
    """capacity = count + 5: an empty pair, one lane, either side of a wave and of a work-group's chunk"""
    stats = check(gpu_lib, nc.count_case(n))
    assert n < 63 or stats["n_new"][0] > 0


def test_three_pairs_on_one_keyframe_and_one_reversed(gpu_lib):
    """kc.PAIRS on four keyframes of 65 features: the claim rule across three pairs; the reversed pair shares no keyframe 1"""
    case = nc.count_case(65, 4, tuple(kc.PAIRS))
    stats = check(gpu_lib, case)
    assert stats["n_verdict"][1:3, nr.CLAIMED].sum() > 0 and stats["n_verdict"][[0, 3], nr.CLAIMED].sum() == 0


@pytest.mark.parametrize("enabled", [[0, 1, 1], [1, 0, 1], [0, 0, 0]])
def test_a_disabled_pair(gpu_lib, enabled):
    """zero stats and a row of -1; what it would have accepted is not claimed behind it; its d_new row keeps the poison"""
    check(gpu_lib, dict(nc.hand_cases()["claimed"], enabled=enabled))
    check(gpu_lib, dict(nc.count_case(65, 4, tuple(kc.PAIRS)), enabled=enabled + [1]))


def test_without_the_optional_arrays(gpu_lib):
    """d_verdict NULL; d_kps_raw NULL: UnprojectStereo reads d_kps; d_u_right NULL: every feature is mono.  One handle, used again."""
    mt = gpu_lib.OrbMatcher()
    for case in (nc.random_case(5, "forward"), nc.hand_cases()["unprojected_1_raw_keys"]):
        check(gpu_lib, case, with_verdict=False, mt=mt)
        full = check(gpu_lib, case, mt=mt)
        no_raw = check(gpu_lib, case, with_raw=False, mt=mt)
        mono = check(gpu_lib, case, with_right=False, mt=mt)
        unprojected = [nr.UNPROJECTED_1, nr.UNPROJECTED_2]
        assert mono["n_verdict"][:, unprojected].sum() == 0 and full["n_verdict"][:, unprojected].sum() > 0
        assert no_raw["n_verdict"][:, unprojected].sum() > 0
    mt.close()


def test_search_then_new_points_on_the_device(gpu_lib, ob, synth):
    """amos_match_triangulation_batch_device and amos_match_new_points_batch_device back to back on one stream, no synchronisation and no
    copy between them, on the 160 x 120 synth keyframes with kc.PAIRS == the CPU oracle's search + the restatement"""
    import torch
    case = nc.synth_case(ob, synth)
    sides, cams, pairs, lv = case["sides"], case["cams"], case["pairs"], case["levels"]
    geos = [gpu_lib.kf_geometry_from_poses(cams[a], cams[b]) for a, b in pairs]
    assert all(ok for _, ok in geos)
    geos = [g for g, _ in geos]
    cap = max(len(s["desc"]) for s in sides) + 5
    a = kc.pack(sides, cap)
    b = hnb.pack(dict(case, match=[np.zeros(0, np.int32)] * len(pairs)), pad=5)
    assert b["capacity"] == cap
    d = {k: _up(v) for k, v in a.items()}
    d_depth = _up(b["depth"])
    d_1, d_2 = _up(np.array([p[0] for p in pairs], np.int32)), _up(np.array([p[1] for p in pairs], np.int32))
    d_geo, d_sf, d_sg = _up(np.stack(geos)), _up(lv[0]), _up(lv[1])
    d_match = torch.full((len(pairs), cap), 12345, dtype=torch.int32, device="cuda")
    d_sstats = torch.full((len(pairs), 4), -9, dtype=torch.int32, device="cuda")
    d_new, d_verdict, d_stats = outputs(len(pairs), cap)
    torch.cuda.synchronize()
    mt = gpu_lib.OrbMatcher()
    mt.triangulation_batch_device(d["kps"].data_ptr(), d["desc"].data_ptr(), d["counts"].data_ptr(), d["n_nodes"].data_ptr(), d["node_ids"].data_ptr(),
                                  d["node_off"].data_ptr(), d["node_idx"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(), len(pairs), cap, d_geo.data_ptr(),
                                  d_sf.data_ptr(), d_sg.data_ptr(), len(lv[0]), d_match.data_ptr(), d_sstats.data_ptr(), only_stereo=False,
                                  check_orientation=True, d_has_point=d["has_point"].data_ptr(), d_u_right=d["u_right"].data_ptr())
    mt.new_points_batch_device(d["kps"].data_ptr(), d["counts"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(), pairs, cap, d_match.data_ptr(),
                               d_sf.data_ptr(), d_sg.data_ptr(), len(lv[0]), np.stack(cams), d_new.data_ptr(), d_stats.data_ptr(),
                               d_verdict=d_verdict.data_ptr(), d_u_right=d["u_right"].data_ptr(), d_depth=d_depth.data_ptr())
    mt.sync()
    new, verdict, stats = fetch(d_new, d_verdict, d_stats, len(pairs), cap)
    match = d_match.cpu().numpy()
    mt.close()
    rows = []
    for p, ((i1, i2), g) in enumerate(zip(pairs, geos)):
        want_n, want = kc.oracle_triangulation(sides[i1], sides[i2], g, lv[0], lv[1], 0, 1)
        assert np.array_equal(match[p, :len(want)], want) and (match[p, len(want):] == -1).all()
        rows.append(want)
    want_new, want_verdict, want_stats = hnb.expected(dict(case, match=rows), cap)
    print("verdicts per pair:", want_stats["n_verdict"].tolist())
    assert stats.tobytes() == want_stats.tobytes() and verdict.tobytes() == want_verdict.tobytes() and new.tobytes() == want_new.tobytes()
    assert want_stats["n_new"].sum() > 0 and want_stats["n_verdict"][1:3, nr.CLAIMED].sum() > 0


def test_a_bad_pair_slot_on_the_device(gpu_lib):
    """the host slots pass the check, the device arrays name a frame outside: the pair writes zero stats with status bit 2 and reads nothing"""
    import torch
    case = nc.hand_cases()["triangulated"]
    a = hnb.pack(case, 6)
    cap = a["capacity"]
    d = {k: _up(a[k]) for k in ("kps", "counts", "match", "scale", "sigma2")}
    d_1, d_2 = _up(np.array([0], np.int32)), _up(np.array([7], np.int32))
    d_new, d_verdict, d_stats = outputs(1, cap)
    torch.cuda.synchronize()
    mt = gpu_lib.OrbMatcher()
    mt.new_points_batch_device(d["kps"].data_ptr(), d["counts"].data_ptr(), d_1.data_ptr(), d_2.data_ptr(), a["pairs"], cap, d["match"].data_ptr(),
                               d["scale"].data_ptr(), d["sigma2"].data_ptr(), len(a["scale"]), a["cams"], d_new.data_ptr(), d_stats.data_ptr(),
                               d_verdict=d_verdict.data_ptr())
    mt.sync()
    new, verdict, stats = fetch(d_new, d_verdict, d_stats, 1, cap)
    mt.close()
    assert (verdict == -1).all() and stats["status"][0] == gpu_lib.NEW_POINTS_BAD_SLOT and stats["n_matches"][0] == 0 and stats["n_new"][0] == 0
    assert new.tobytes() == np.full((1, cap), np.array(hnb.POISON_NEW, nr.NEW_POINT), nr.NEW_POINT).tobytes()
