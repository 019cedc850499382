"""Relocalization's SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) without a GPU: the plain-Python restatement
(tests/reloc_restatement.py) against the reference-side prefilter + the CPU oracle's loop on seeded scenes, hand cases whose expected
values are worked out in their docstrings, and the new entry points of the library with every argument they refuse."""
import ctypes as C

import numpy as np
import pytest

import adaptor_prefilter as ap
import host_binding as hb
import motion_model_restatement as mr
import reloc_restatement as rr

f32 = np.float32
SCENES = {"small": (320, 240, 500, 4, 260.0), "large": (640, 480, 1000, 8, 520.0)}  # width, height, features, levels, focal length


@pytest.fixture(scope="module")
def scenes(ob, synth):
    out = {}
    for name, (w, h, nf, nl, focal) in SCENES.items():
        orc = ob.Oracle(nf, 1.2, nl)
        frames = [orc.extract(synth.frame(3, k, h, w)) for k in range(2)]
        out[name] = dict(frames=frames, sf=orc.tables()["scale"], bounds=(0.0, float(w), 0.0, float(h)), intr=(focal, focal, w / 2.0, h / 2.0))
    return out


def oracle_search(kps, desc, points, cam, found, match_in, sf, bounds):
    """adaptor_prefilter.reloc_queries + orc_search_by_projection_kf; the query indices of the new matches mapped back to point indices.
    -> (n, match, queries, point index of every query)"""
    T = np.eye(4, dtype=f32)
    T[:3, :3], T[:3, 3] = cam["Rcw"].reshape(3, 3), cam["tcw"]
    tc = hb.test_camera(T, sf, float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), bounds=tuple(float(b) for b in bounds))
    ok = ((points["flags"] & rr.SKIP) == 0) & (np.asarray(found) == 0)
    q, pidx = ap.reloc_queries(hb, tc, T, points["pos"], points["min_distance"], points["max_distance"], points["desc"], np.arange(len(points)),
                               ok, points["angle"], sf[1], len(sf))
    view, keep = hb.frame_view(kps, desc, None, tuple(float(b) for b in bounds))
    n, m = hb.search_kf("oracle", view, q, match_in, sf, float(cam["th"]), int(cam["orb_dist"]), check_ori=bool(cam["check_orientation"]))
    new = (np.asarray(match_in) < 0) & (m >= 0)
    m[new] = pidx[m[new]]
    return n, m, q, pidx


@pytest.mark.parametrize("check_ori", [1, 0])
@pytest.mark.parametrize("th,orb_dist", rr.PARAMS)
@pytest.mark.parametrize("size", ["small", "large"])
def test_restatement_equals_prefilter_and_oracle(scenes, size, th, orb_dist, check_ori):
    sc = scenes[size]
    (kps, desc), (kkps, kdesc) = sc["frames"]
    rng = np.random.default_rng(len(size) * 100 + int(th))
    points = rr.make_points(rng, kkps, kdesc, len(kkps), rr.KF_POSE, sc["intr"], sc["sf"])
    match_in, found = rr.entry_state(rng, len(kps), len(points))
    cur = mr.moved(rr.KF_POSE, **rr.CUR_MOTIONS[0])
    cam = rr.camera(*cur, *sc["intr"], th=th, orb_dist=orb_dist, check_orientation=check_ori)
    got = rr.search(kps, desc, points, cam, found, match_in, sc["sf"], sc["bounds"])
    n, m, q, pidx = oracle_search(kps, desc, points, cam, found, match_in, sc["sf"], sc["bounds"])
    print(size, th, orb_dist, check_ori, {k: got[k] for k in rr.STAT_FIELDS}, "oracle", n)
    assert np.array_equal(np.nonzero(got["projected"])[0], pidx)
    for name in ("u", "v", "level", "angle", "desc"):
        assert got["query"][name][pidx].tobytes() == q[name].tobytes(), name
    assert got["n_matches"] == n and np.array_equal(got["match"], m)
    assert np.array_equal(got["match"][match_in >= 0], match_in[match_in >= 0])  # the entry matches stand
    third, fifth = len(kps) / 3.0, len(points) / 5.0
    assert 0.8 * third < got["n_occupied"] < 1.2 * third and 0.6 * fifth < got["n_found"] < 1.3 * fifth
    assert got["n_matches"] > 20 and got["status"] == 0
    assert got["projected"][0] == 1 or (points["flags"][0] & rr.SKIP) or found[0]  # point 0 lies behind the camera: searched all the same


def two_close():
    """The hand frame with feature 1 moved 4 px beside feature 0 (one window at th = 3: radius 3 * 1.728 = 5.2 px on level 3) and given
    feature 0's descriptor with bits 100 .. 109 flipped."""
    kps, desc = rr.hand_frame()
    kps["x"][1], kps["y"][1] = kps["x"][0] + 4.0, kps["y"][0]
    desc[1] = desc[0]
    for b in range(100, 110):
        desc[1][b // 8] ^= 1 << (b % 8)
    return kps, desc


def run(kps, desc, points, match_in=None, found=None, **kw):
    kw.setdefault("th", 3.0)
    kw.setdefault("orb_dist", 64)
    kw.setdefault("check_orientation", 0)
    m = np.full(len(kps), -1, np.int32) if match_in is None else match_in
    return rr.search(kps, desc, np.concatenate(points), rr.hand_camera(**kw), found, m, rr.HAND_SCALE, rr.HAND_BOUNDS)


def test_hand_projection():
    """Feature 0 sits at (60, 60): the point ((60 - 320) / 512, (60 - 240) / 512, 1) is exact in float32 and projects to u = 512 * x + 320 = 60,
    v = 60.  dist3D = sqrt(0.5078^2 + 0.3516^2 + 1) = 1.1755; 2.0 / 1.1755 = 1.701 exceeds 1, 1.2 and 1.44 of the table, not 1.728: level 3."""
    kps, desc = two_close()
    r = run(kps, desc, [rr.hand_point(kps, desc, 0)])
    assert (r["query"]["u"][0], r["query"]["v"][0], r["query"]["level"][0], r["projected"][0]) == (60.0, 60.0, 3, 1)
    assert rr.predict_level(2.0, 1.1755, rr.HAND_SCALE) == 3 and rr.predict_level(2.0, 1.0, rr.HAND_SCALE) == 4
    assert rr.predict_level(100.0, 1.0, rr.HAND_SCALE) == 7 and rr.predict_level(0.5, 1.0, rr.HAND_SCALE) == 0


def test_a_best_occupied_on_entry_takes_the_second():
    """The point carries feature 0's descriptor: distances 0 (feature 0) and 10 (feature 1).  Feature 0 is set on entry, so the only free
    candidate is feature 1 at 10 <= 64: match[1] = 0, feature 0 keeps its entry value 5, one match, one occupied, nothing re-searched."""
    kps, desc = two_close()
    m = np.full(len(kps), -1, np.int32)
    m[0] = 5
    r = run(kps, desc, [rr.hand_point(kps, desc, 0)], m)
    assert (r["match"][0], r["match"][1], r["n_matches"], r["n_occupied"], r["n_researched"]) == (5, 0, 1, 1, 0)
    assert (r["match"][2:] == -1).all()


def test_b_every_candidate_occupied_is_no_match():
    """Both features of the window are set on entry: bestDist stays 256 > 64, nothing is written."""
    kps, desc = two_close()
    m = np.full(len(kps), -1, np.int32)
    m[0], m[1] = 5, 6
    r = run(kps, desc, [rr.hand_point(kps, desc, 0)], m)
    assert r["n_matches"] == 0 and np.array_equal(r["match"], m) and (r["n_projected"], r["n_occupied"]) == (1, 2)


def test_c_a_found_point_is_never_searched():
    """A (distance 0 to feature 0) is found; B (two bits off: 2 to feature 0, 12 to feature 1) is not.  A is no candidate, so B takes feature 0
    although A would have won it: match[0] = 1 (B's index), one candidate, one found."""
    kps, desc = two_close()
    pts = [rr.hand_point(kps, desc, 0), rr.hand_point(kps, desc, 0, flip_bits=2)]
    r = run(kps, desc, pts, found=np.array([1, 0], np.uint8))
    assert (r["match"][0], r["match"][1], r["n_matches"], r["n_candidates"], r["n_found"], r["n_projected"]) == (1, -1, 1, 1, 1, 1)
    assert r["projected"][0] == 0


def test_d_an_earlier_point_takes_the_best():
    """A takes feature 0 (distance 0).  B finds its best, feature 0 (2), set by A and takes its second, feature 1 (12).  No re-search: the
    second of the entry record is free."""
    kps, desc = two_close()
    r = run(kps, desc, [rr.hand_point(kps, desc, 0), rr.hand_point(kps, desc, 0, flip_bits=2)])
    assert (r["match"][0], r["match"][1], r["n_matches"], r["n_researched"]) == (0, 1, 2, 0)


def test_e_three_points_contend_for_two_features():
    """A takes feature 0, B feature 1.  C (three bits off) finds its entry best (feature 0, 3) and entry second (feature 1, 13) both taken,
    searches again and finds nothing: two matches, n_researched = 1."""
    kps, desc = two_close()
    pts = [rr.hand_point(kps, desc, 0), rr.hand_point(kps, desc, 0, flip_bits=2), rr.hand_point(kps, desc, 0, flip_bits=3)]
    r = run(kps, desc, pts)
    assert (r["match"][0], r["match"][1], r["n_matches"], r["n_researched"], r["n_projected"]) == (0, 1, 2, 1, 3)
    assert (r["match"][2:] == -1).all()


def test_f_best_dist_equal_to_orb_dist_is_accepted():
    """64 flipped bits are a distance of 64: accepted with ORBdist = 64 (bestDist <= ORBdist), rejected with 63; 65 bits are rejected with 64."""
    kps, desc = rr.hand_frame()
    at = [rr.hand_point(kps, desc, 10, flip_bits=64)]
    assert run(kps, desc, at, orb_dist=64)["match"][10] == 0 and run(kps, desc, at, orb_dist=64)["n_matches"] == 1
    assert run(kps, desc, at, orb_dist=63)["n_matches"] == 0
    r = run(kps, desc, [rr.hand_point(kps, desc, 10, flip_bits=65)], orb_dist=64)
    assert r["n_matches"] == 0 and (r["match"] == -1).all() and r["n_projected"] == 1


def test_g_the_distance_range_is_strict_on_both_sides():
    """A point on the optical axis at depth z has dist3D = z exactly (Ow = 0).  z = 0.8f * 1.25f: dist3D < 0.8f * min is false, kept; with
    min one ulp larger it is dropped.  z = 1.2f * 2.0f: dist3D > 1.2f * max is false, kept; with max one ulp smaller it is dropped."""
    kps, desc = rr.hand_frame()
    kps["x"][0], kps["y"][0] = 320.0, 240.0
    z_min, z_max = f32(0.8) * f32(1.25), f32(1.2) * f32(2.0)
    up, down = np.nextafter(f32(1.25), f32(2)), np.nextafter(f32(2.0), f32(0))
    cases = [(z_min, (1.25, 4.0), 1), (z_min, (up, 4.0), 0), (z_max, (0.5, 2.0), 1), (z_max, (0.5, down), 0)]
    for z, rng_, want in cases:
        r = run(kps, desc, [rr.hand_point(kps, desc, 0, z=z, dist_range=rng_)], th=10.0)
        assert (r["query"]["u"][0], r["query"]["v"][0]) == ((320.0, 240.0) if want else (0.0, 0.0))
        assert (r["projected"][0], r["n_projected"], r["n_candidates"]) == (want, want, 1), (z, rng_)


def test_h_a_point_behind_the_camera_is_searched():
    """(-x, -y, -1) has zc = -1, invzc = -1 and u = (512 * -x) * -1 + 320: the projection of (x, y, 1).  There is no invzc < 0 test, so the
    point is searched and matched (the motion-model search would skip it)."""
    kps, desc = rr.hand_frame()
    p = rr.hand_point(kps, desc, 10, z=-1.0)
    assert p["pos"][0, 2] == -1.0
    r = run(kps, desc, [p])
    assert (r["query"]["u"][0], r["query"]["v"][0]) == (kps["x"][10], kps["y"][10])
    assert (r["projected"][0], r["match"][10], r["n_matches"], r["status"]) == (1, 0, 1, 0)


def test_i_zero_depth_sets_the_status_bit_and_nothing_else():
    """zc = 0: invzc = inf, u = (512 * 0.1) * inf + 320 = inf (and 0 * inf = NaN for the point at the origin): not finite, bit 0."""
    kps, desc = rr.hand_frame()
    for pos in ([0.1, 0.1, 0.0], [0.0, 0.0, 0.0]):
        p = rr.hand_point(kps, desc, 10)
        p["pos"] = pos
        r = run(kps, desc, [p])
        assert (r["status"], r["n_candidates"], r["n_projected"], r["n_matches"], r["projected"][0]) == (1, 1, 0, 0, 0)
        assert (r["match"] == -1).all()


def test_j_a_losing_bin_clears_only_this_calls_matches():
    """Eleven points with rot = 0 (bin 0) on features 20 .. 30 and point 0 with rot = 96 (bin 8) on feature 0: max1 = 11 and 1 < 0.1f * 11, so
    bin 8 loses and feature 0 is cleared: 12 - 1 = 11.  Feature 1, 4 px beside it and set on entry (to point 0 itself, the very point of the
    losing bin, as SearchByBoW might have left it), is in no histogram entry of this call and stays.  Without the check all twelve stand."""
    kps, desc = two_close()
    pts = [rr.hand_point(kps, desc, 0, angle=96.0)] + [rr.hand_point(kps, desc, f) for f in range(20, 31)]
    assert mr.rotation_bin(96.0, 0.0) == 8
    m = np.full(len(kps), -1, np.int32)
    m[1] = 0
    r = run(kps, desc, pts, m, check_orientation=1)
    assert (r["match"][0], r["match"][1], r["n_matches"], r["n_occupied"]) == (-1, 0, 11, 1)
    assert list(r["match"][20:31]) == list(range(1, 12)) and (r["match"] >= 0).sum() == 12
    r = run(kps, desc, pts, m, check_orientation=0)
    assert (r["match"][0], r["match"][1], r["n_matches"]) == (0, 0, 12) and list(r["match"][20:31]) == list(range(1, 12))


def test_found_from_match_equals_the_explicit_array(scenes):
    sc = scenes["small"]
    (kps, desc), (kkps, kdesc) = sc["frames"]
    rng = np.random.default_rng(77)
    points = rr.make_points(rng, kkps, kdesc, len(kkps), rr.KF_POSE, sc["intr"], sc["sf"])
    match_in, found = rr.entry_state(rng, len(kps), len(points))
    cur = mr.moved(rr.KF_POSE, **rr.CUR_MOTIONS[0])
    explicit = found.copy()
    explicit[match_in[match_in >= 0]] = 1
    assert explicit.sum() > found.sum() + 50
    a = rr.search(kps, desc, points, rr.camera(*cur, *sc["intr"], found_from_match=1), found, match_in, sc["sf"], sc["bounds"])
    b = rr.search(kps, desc, points, rr.camera(*cur, *sc["intr"], found_from_match=0), explicit, match_in, sc["sf"], sc["bounds"])
    c = rr.search(kps, desc, points, rr.camera(*cur, *sc["intr"], found_from_match=0), found, match_in, sc["sf"], sc["bounds"])
    assert np.array_equal(a["match"], b["match"]) and np.array_equal(a["projected"], b["projected"])
    assert [a[k] for k in rr.STAT_FIELDS] == [b[k] for k in rr.STAT_FIELDS]
    assert a["n_found"] > c["n_found"] and not np.array_equal(a["match"], c["match"])


def test_library_exports_the_reloc_entry_points(pkg):
    names = ("amos_match_reloc_batch_device", "amos_match_reloc")
    L = C.CDLL(pkg.LIB_PATH)
    for name in names:
        assert name in pkg.EXPORTS and hasattr(L, name), name
    assert hasattr(pkg.OrbMatcher, "reloc_batch_device") and hasattr(pkg.OrbMatcher, "reloc")
    assert (pkg.RELOC_POINT_DTYPE.itemsize, pkg.RELOC_CAMERA_DTYPE.itemsize, pkg.RELOC_STATS_DTYPE.itemsize, pkg.KF_QUERY_DTYPE.itemsize) == (64, 84, 32, 48)
    assert (C.sizeof(pkg.RelocPoint), C.sizeof(pkg.RelocCamera), C.sizeof(pkg.RelocStats)) == (64, 84, 32)
    assert pkg.RELOC_POINT_DTYPE == rr.POINT and pkg.RELOC_CAMERA_DTYPE == rr.CAMERA and pkg.KF_QUERY_DTYPE == hb.KF_QUERY
    assert pkg.RELOC_POINT_DTYPE.fields["flags"][1] == 24  # what the pose kernel is given as flags_offset
    assert tuple(pkg.RELOC_STATS_DTYPE.names) == rr.STAT_FIELDS


def test_invalid_arguments_return_before_the_device_is_touched(pkg):
    """No GPU here: every refusal comes back as AMOS_ERR_INVALID (-1) with the entry's name in the message; the handle is a dummy that is
    read only after the checks have passed."""
    L = pkg.lib()
    fake = C.create_string_buffer(1024)
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    sf = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)])).astype(f32)
    base = dict(d_kps=p, d_desc=p, d_counts=p, d_cell_start=p, d_items=p, d_points=p, d_found=None, d_pose=None, d_query=p, d_projected=p,
                d_match=p, d_stats=p, n_frames=2, capacity=100, bounds=(0.0, 640.0, 0.0, 480.0), fop=[0, 1, 0], off=[0, 10, 10, 30], sf=sf,
                cams=[rr.hand_camera() for _ in range(3)])

    def call(handle=fake, **kw):
        a = dict(base, **kw)
        fop, off = np.asarray(a["fop"], np.int32), np.asarray(a["off"], np.int32)
        cams = np.array(a["cams"], rr.CAMERA)
        s = pkg.RelocSearch(a["d_kps"], a["d_desc"], a["d_counts"], a["d_cell_start"], a["d_items"], a["d_points"],
                            None if a.get("no_fop") else fop.ctypes.data, None if a.get("no_off") else off.ctypes.data,
                            None if a.get("no_cams") else cams.ctypes.data, a["d_found"], a["d_pose"],
                            None if a.get("no_sf") else a["sf"].ctypes.data, a["d_query"], a["d_projected"], a["d_match"], a["d_stats"],
                            a["n_frames"], a.get("n_pairs", len(cams)), a["capacity"], a.get("n_levels", len(a["sf"])), *a["bounds"])
        rc = L.amos_match_reloc_batch_device(handle, C.byref(s))
        if rc == -1:
            assert b"amos_match_reloc_batch_device" in L.amos_last_error()
        return rc
    assert call(handle=None) == -1 and L.amos_match_reloc_batch_device(fake, None) == -1
    for name in ("d_kps", "d_desc", "d_counts", "d_cell_start", "d_items", "d_points", "d_query", "d_projected", "d_match", "d_stats"):
        assert call(**{name: None}) == -1, name
    for name in ("no_fop", "no_off", "no_cams", "no_sf"):
        assert call(**{name: True}) == -1, name
    assert call(n_pairs=0) == -1 and call(n_frames=0) == -1
    assert call(capacity=0) == -1 and call(capacity=65537) == -1
    assert call(n_levels=0) == -1 and call(n_levels=1000) == -1
    assert call(fop=[0, 2, 0]) == -1 and call(fop=[0, -1, 0]) == -1
    assert call(off=[0, 10, 9, 30]) == -1 and call(off=[-1, 10, 10, 30]) == -1
    assert call(bounds=(0.0, 0.0, 0.0, 480.0)) == -1 and call(bounds=(0.0, 640.0, 480.0, 0.0)) == -1
    for bad in (dict(orb_dist=256), dict(orb_dist=-1), dict(th=0.0), dict(th=-1.0), dict(th=np.inf), dict(th=np.nan)):
        cams = [rr.hand_camera(), rr.hand_camera(**bad), rr.hand_camera()]
        assert call(cams=cams) == -1, bad
    # the host form
    kp, d = np.zeros(4, pkg.KP_DTYPE), np.zeros((4, 32), np.uint8)
    pts, q, pj = np.zeros(2, rr.POINT), np.zeros(2, pkg.KF_QUERY_DTYPE), np.zeros(2, np.uint8)
    m, st = np.full(4, -1, np.int32), np.zeros(1, pkg.RELOC_STATS_DTYPE)

    def host(handle=fake, kps=kp, desc=d, n=4, points=pts, n_points=2, cam=rr.hand_camera(), sf_=sf, n_levels=8, bounds=(0.0, 640.0, 0.0, 480.0),
             query=q, projected=pj, match=m, stats=st):
        cam = None if cam is None else np.array([cam], rr.CAMERA)
        rc = L.amos_match_reloc(handle, pkg._p(kps), pkg._p(desc), n, pkg._p(points), n_points, None, pkg._p(cam), pkg._p(sf_), n_levels,
                                *bounds, pkg._p(query), pkg._p(projected), pkg._p(match), pkg._p(stats))
        if rc == -1:
            assert b"amos_match_reloc:" in L.amos_last_error()
        return rc
    assert host(handle=None) == -1 and host(cam=None) == -1 and host(sf_=None) == -1 and host(stats=None) == -1
    assert host(n=-1) == -1 and host(n=65537) == -1 and host(n_points=-1) == -1
    assert host(kps=None) == -1 and host(desc=None) == -1 and host(match=None) == -1
    assert host(points=None) == -1 and host(query=None) == -1 and host(projected=None) == -1
    assert host(n_levels=0) == -1 and host(bounds=(0.0, 640.0, 5.0, 5.0)) == -1
    assert host(cam=rr.hand_camera(orb_dist=256)) == -1 and host(cam=rr.hand_camera(th=np.nan)) == -1 and host(cam=rr.hand_camera(th=0.0)) == -1
