"""The frame front end on the device at every camera the reference ships (tests/golden/ref_settings, read by tests/ref_settings.py), bit for
bit against the CPU oracle in the style of tests/test_gpu_parity.py: the ORB tables and the extraction with the file's ORB parameters,
UndistortKeyPoints with the file's coefficient list at its own length, ComputeImageBounds, ComputeStereoFromRGBD on 16-bit depth with the
file's 1 / DepthMapFactor and bf (RGB-D) or the grid cells alone (Monocular) on the undistorted keypoints and the camera's bounds,
AssignFeaturesToGrid against a numpy counting sort, and ComputeStereoMatches (Stereo) with the file's bf and min_z = bf / fx on a pair whose
bottom half lies 400 px (KITTI) or 200 px (EuRoC) apart, against tests/stereo_restatement.py.  Then hand cameras on 640 x 480 for the
branches no shipped file takes.  Two synthetic frames of the case's size per case, every device result computed once per case."""
import numpy as np
import pytest

import ref_settings as rs
import stereo_restatement as sr
from test_gpu_parity import _same

pytestmark = pytest.mark.gpu

CASES = {rs.case_id(s): s for s in rs.cases()}
STEREO_BOTTOM = {"KITTI": (400, 448), "EuRoC": (200, 256)}  # bottom-half disparity, margin of the pair
GRID_CELLS = 64 * 48
f32 = np.float32


def wide_stereo_pair(synth, stream, h, w, d_top, d_bot, seed, margin):
    """stereo_restatement.stereo_pair cut from a frame `margin` columns wider than the left image instead of its fixed 64, which no
    disparity can exceed: the top half of the right image sees disparity d_top, the bottom half d_bot; +-2 seeded noise on the right."""
    assert 0 <= d_top <= margin and 0 <= d_bot <= margin
    wide = synth.frame(stream, 0, h, w + margin)
    left = np.ascontiguousarray(wide[:, :w])
    right = np.concatenate([wide[:h // 2, d_top:d_top + w], wide[h // 2:, d_bot:d_bot + w]]).astype(np.int64)
    right = right + np.random.default_rng(seed).integers(-2, 3, size=right.shape)
    return left, np.clip(right, 0, 255).astype(np.uint8)


def case_frames(synth, s):
    """(n, h, w) frames of a case: two frames of the synth stream, or for Stereo the left and the right image of one pair."""
    if s.sensor == "Stereo":
        d_bot, margin = next(v for k, v in STEREO_BOTTOM.items() if s.name.startswith(k))
        return np.stack(wide_stereo_pair(synth, 3, s.height, s.width, 12, d_bot, 99, margin))
    return synth.frames(3, 0, 2, s.height, s.width)


def case_depth(s, n):
    """raw 16-bit depth maps, a quarter of the pixels without a reading"""
    rng = np.random.default_rng(s.width + len(s.name))
    raw = rng.integers(0, 30000, (n, s.height, s.width)).astype(np.uint16)
    raw[rng.random(raw.shape) < 0.25] = 0
    return raw


def counting_sort(cell):
    """Frame::AssignFeaturesToGrid as a CSR: (start [64 * 48 + 1], items = the keypoints inside the grid, by cell, ascending inside a cell)"""
    inside = np.nonzero(cell >= 0)[0]
    start = np.concatenate([[0], np.cumsum(np.bincount(cell[inside], minlength=GRID_CELLS))]).astype(np.int32)
    return start, inside[np.argsort(cell[inside], kind="stable")].astype(np.int32)


def device_front(pkg, frames, orb, intr, dist, bf=None, raw_depth=None, inv_factor=1.0, stereo_min_z=None):
    """extract -> undistort -> bounds -> glue / cells -> grid build (-> stereo match of frames 0, 1) on one resident batch."""
    import torch
    n, h, w = frames.shape
    ext = pkg.OrbExtractor(max_width=w, max_height=h, max_batch=n, **orb)
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    torch.cuda.synchronize()
    ext.extract_batch_device(d_frames.data_ptr(), h * w, w, w, h, n)
    _, _, d_counts, cap = ext.batch_results_device()
    d_un = torch.zeros((n, cap, 7), dtype=torch.float32, device="cuda")
    d_ur = torch.full((n, cap), 7.0, dtype=torch.float32, device="cuda")
    d_dep = torch.full((n, cap), 7.0, dtype=torch.float32, device="cuda")
    d_cell = torch.full((n, cap), -5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bounds = pkg.image_bounds(w, h, *intr, dist)
    ext.undistort_batch_device(*intr, dist, d_un.data_ptr())
    if raw_depth is not None:
        d_raw = torch.from_numpy(raw_depth.view(np.int16)).cuda()
        torch.cuda.synchronize()
        ext.rgbd_glue_batch_device(d_raw.data_ptr(), True, inv_factor, h * w * 2, w * 2, bf, bounds, d_ur.data_ptr(), d_dep.data_ptr(),
                                   d_cell.data_ptr(), d_kps_un=d_un.data_ptr())
    else:
        ext.rgbd_glue_batch_device(None, False, 1.0, 0, 0, 0.0, bounds, None, None, d_cell.data_ptr(), d_kps_un=d_un.data_ptr())
    out = dict(tables=ext.tables(), bounds=bounds, cap=cap)
    if stereo_min_z is not None:
        st = [torch.full((1, cap), 7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        st += [torch.full((1, cap), 7, dtype=torch.int32, device="cuda"), torch.full((1,), 7, dtype=torch.int32, device="cuda")]
        torch.cuda.synchronize()
        ext.stereo_match_batch_device(None, 1, bf, stereo_min_z, *(t.data_ptr() for t in st))
    ext.sync()
    mt = pkg.OrbMatcher()
    d_start = torch.full((n, GRID_CELLS + 1), -5, dtype=torch.int32, device="cuda")
    d_items = torch.full((n, cap), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mt.grid_build_batch_device(d_cell.data_ptr(), d_counts, n, cap, d_start.data_ptr(), d_items.data_ptr())
    mt.sync()
    torch.cuda.synchronize()
    out["frames"] = [ext.batch_fetch(f) for f in range(n)]
    out["un"] = d_un.cpu().numpy().view(np.uint8).reshape(n, cap, 28)
    out.update(ur=d_ur.cpu().numpy(), dep=d_dep.cpu().numpy(), cell=d_cell.cpu().numpy(), start=d_start.cpu().numpy(), items=d_items.cpu().numpy())
    if stereo_min_z is not None:
        out["stereo"] = [t.cpu().numpy() for t in st]
    mt.close()
    return out


def oracle_front(ob, frames, orb, intr, dist, bf=None, raw_depth=None, inv_factor=1.0):
    n, h, w = frames.shape
    orc = ob.Oracle(**orb)
    out = dict(tables=orc.tables(), bounds=ob.image_bounds(w, h, *intr, dist), frames=[], un=[], glue=[])
    for f in range(n):
        kps, desc = orc.extract(frames[f])
        kps, desc = kps.copy(), desc.copy()
        un = kps.copy()
        if len(kps):
            xy = ob.undistort_points(np.stack([kps["x"], kps["y"]], 1), *intr, dist)
            un["x"], un["y"] = xy[:, 0], xy[:, 1]
        if raw_depth is not None:
            depth = (raw_depth[f].astype(f32) * f32(inv_factor)).astype(f32)  # Tracking's convertTo(CV_32F, mDepthMapFactor)
            glue = ob.rgbd_glue(kps, depth, bf, out["bounds"], kps_un=un)
        else:
            glue = (None, None, ob.rgbd_glue(kps, np.zeros((h, w), f32), 1.0, out["bounds"], kps_un=un)[2])
        out["frames"].append((kps, desc))
        out["un"].append(un)
        out["glue"].append(glue)
    return out


def assert_front(ob, got, want, with_depth):
    """every comparison of the front end that both sides have; -> number of keypoints outside the grid (cell -1), per frame"""
    for k in want["tables"]:
        _same(got["tables"][k], want["tables"][k], k)
    assert got["bounds"] == want["bounds"], (got["bounds"], want["bounds"])
    outside = []
    for f, ((kg, dg), (ko, do)) in enumerate(zip(got["frames"], want["frames"])):
        _same(kg, ko, f"frame {f} keypoints")
        _same(dg, do, f"frame {f} descriptors")
        m = len(ko)
        _same(np.frombuffer(got["un"][f, :m].tobytes(), ob.KP_DTYPE), want["un"][f], f"frame {f} mvKeysUn")
        ur, dep, cell = want["glue"][f]
        _same(got["cell"][f, :m], cell, f"frame {f} grid cell")
        if with_depth:
            _same(got["ur"][f, :m], ur, f"frame {f} mvuRight")
            _same(got["dep"][f, :m], dep, f"frame {f} mvDepth")
            assert (ur > 0).sum() > m // 2
        start, items = counting_sort(cell)
        _same(got["start"][f], start, f"frame {f} cell starts")
        _same(got["items"][f, :len(items)], items, f"frame {f} grid items")
        assert len(items) == m - (cell < 0).sum()
        outside.append(int((cell < 0).sum()))
    return outside


@pytest.fixture(scope="module")
def fronts(gpu_lib, ob, synth):
    """case id -> (settings, frames, device results, oracle results), each computed on first use"""
    done = {}

    def get(cid):
        if cid not in done:
            s = CASES[cid]
            frames = case_frames(synth, s)
            kw = dict(orb=rs.orb_kwargs(s), intr=rs.intrinsics(s), dist=rs.dist_array(s))
            if s.sensor == "RGB-D":
                kw.update(bf=float(s.bf), raw_depth=case_depth(s, len(frames)), inv_factor=rs.inv_depth_factor(s))
            want = oracle_front(ob, frames, **kw)
            if s.sensor == "Stereo":
                kw.update(bf=float(s.bf), stereo_min_z=float(f32(s.bf) / f32(s.fx)))  # Frame.cc: mb = mbf / fx
            done[cid] = (s, frames, device_front(gpu_lib, frames, **kw), want)
        return done[cid]
    return get


def test_every_settings_file_is_a_case():
    assert len(rs.files()) == 16 and len(CASES) >= 12
    assert {s.sensor for s in CASES.values()} == set(rs.SENSORS)
    assert {(s.width, s.height) for s in CASES.values()} == {(640, 480), (752, 480), (1241, 376)}
    assert {len(s.dist) for s in CASES.values()} == {4, 5}


@pytest.mark.parametrize("cid", list(CASES))
def test_front_end_equals_the_oracle(fronts, ob, cid):
    s, frames, got, want = fronts(cid)
    outside = assert_front(ob, got, want, s.sensor == "RGB-D")
    print(cid, "keypoints", [len(k) for k, _ in want["frames"]], "bounds", want["bounds"], "outside the grid", outside)
    assert all(len(k) > 0.9 * s.n_features for k, _ in want["frames"])
    image = (0.0, float(s.width), 0.0, float(s.height))
    if s.dist[0] == 0:  # Frame.cc:1054 and :1123: mvKeysUn = mvKeys, the bounds are the image
        assert want["bounds"] == image and all(_un.tobytes() == k.tobytes() for _un, (k, _) in zip(want["un"], want["frames"]))
    else:
        assert want["bounds"] != image and all(np.abs(_un["x"] - k["x"]).max() > 0.5 for _un, (k, _) in zip(want["un"], want["frames"]))


def test_the_searches_cameras_have_the_bounds_the_tests_name(fronts):
    for name, (sensor, file) in rs.SEARCH_CAMERAS.items():
        b = fronts(f"{sensor}-{file}")[2]["bounds"]
        assert (b[0] > 0 and b[2] > 0) if rs.IMAGE_BOUNDS_SIGN[name] > 0 else (b[0] < 0 and b[2] < 0), (name, b)


def test_fast_threshold_12_differs_from_20(fronts):
    """KITTI04-12's iniThFAST = 12 on the frames that KITTI00-02 extracts with 20: another set of keypoints."""
    (s12, f12, got12, _), (s20, f20, got20, _) = fronts("Stereo-KITTI04-12"), fronts("Stereo-KITTI00-02")
    assert (s12.ini_th, s20.ini_th) == (12, 20) and f12.tobytes() == f20.tobytes()
    print([len(k) for k, _ in got12["frames"]], [len(k) for k, _ in got20["frames"]])
    for (k12, _), (k20, _) in zip(got12["frames"], got20["frames"]):
        assert k12.tobytes() != k20.tobytes()


@pytest.mark.parametrize("cid", [c for c, s in CASES.items() if s.sensor == "Stereo"])
def test_stereo_matches_beyond_64_px(fronts, ob, cid):
    """bf and min_z = bf / fx of the file: KITTI searches up to fx = 707 .. 722 px, EuRoC up to 435 px.  At least 100 accepted matches lie
    more than 64 px apart, the largest disparity the existing pairs reach."""
    s, frames, got, want = fronts(cid)
    (kl, dl), (kr, dr) = got["frames"]
    orb = rs.orb_kwargs(s)
    planes_l, tb = sr.oracle_planes(ob, frames[0], orb["n_features"], orb["scale_factor"], orb["n_levels"])
    planes_r, _ = sr.oracle_planes(ob, frames[1], orb["n_features"], orb["scale_factor"], orb["n_levels"])
    min_z = float(f32(s.bf) / f32(s.fx))
    ur, dep, sad, status, st = sr.compute_stereo_matches(kl, dl, kr, dr, planes_l, planes_r, tb["scale"], tb["inv_scale"], s.height, float(s.bf), min_z)
    disparity = np.where(ur >= 0, kl["x"] - ur, -1)
    print(cid, "matches", int((ur >= 0).sum()), "of", len(kl), "above 64 px", int((disparity > 64).sum()), "largest", float(disparity.max()), st)
    g_ur, g_dep, g_sad, g_status = got["stereo"]
    for g, w_, what in ((g_ur, ur, "u_right"), (g_dep, dep, "depth"), (g_sad, sad, "sad")):
        _same(g[0, :len(kl)], w_, what)
        assert (g[0, len(kl):] == -1).all(), what
    assert int(g_status[0]) == status == 0
    assert (disparity > 64).sum() >= 100 and disparity.max() > STEREO_BOTTOM["KITTI" if s.name.startswith("KITTI") else "EuRoC"][0] - 2


# ---------------------------------------------------------------------------------------------------------------- hand cameras, 640 x 480

TUM1 = rs.read("RGB-D", "TUM1")
EUROC = rs.read("Monocular", "EuRoC")
HAND_ORB = rs.orb_kwargs(TUM1)
PINCUSHION_K1 = (0.1, 0.2, 0.4, 0.8, 1.6)  # tried in this order on the CPU


def hand_camera(ob, synth, name):
    """-> (intrinsics, coefficient list) of a hand camera on TUM1's (or EuRoC's) K"""
    d = rs.dist_array(TUM1)
    if name == "k1_zero":     # Frame.cc:1054: k1 == 0 alone decides, whatever follows it
        return rs.intrinsics(TUM1), np.array([0.0, d[1], d[2], d[3]], f32)
    if name.startswith("len"):
        return rs.intrinsics(TUM1), d[:int(name[3:])].copy()
    if name == "give_up":     # 1 + k1 r^2 < 0 at the corners (r^2 = 0.9 .. 1.0 on EuRoC's K): OpenCV returns the input point
        return rs.intrinsics(EUROC), np.array([-2.5, 0.0, 0.0, 0.0], f32)
    assert name == "pincushion"
    # k1 > 0 alone: undistortion pulls the corners inward further than the middle of an edge, and the bounds come from the corners, so
    # keypoints near the middle of an edge fall outside them (the extractor keeps 16 px from the border, so k1 has to be large): the first
    # k1 of the list at which the ORACLE alone puts at least 10 keypoints of frame 0 outside
    intr = rs.intrinsics(TUM1)
    kps, _ = ob.Oracle(**HAND_ORB).extract(synth.frame(3, 0))
    for k1 in PINCUSHION_K1:
        dist = np.array([k1, 0.0, 0.0, 0.0], f32)
        bounds = ob.image_bounds(640, 480, *intr, dist)
        xy = ob.undistort_points(np.stack([kps["x"], kps["y"]], 1), *intr, dist)
        un = kps.copy()
        un["x"], un["y"] = xy[:, 0], xy[:, 1]
        if (ob.rgbd_glue(kps, np.zeros((480, 640), f32), 1.0, bounds, kps_un=un)[2] < 0).sum() >= 10:
            return intr, dist
    raise AssertionError("no pincushion camera puts 10 keypoints outside the bounds")


@pytest.mark.parametrize("name", ["k1_zero", "len1", "len2", "len3", "give_up", "pincushion"])
def test_hand_camera(gpu_lib, ob, synth, name):
    intr, dist = hand_camera(ob, synth, name)
    frames = synth.frames(3, 0, 2)
    raw = case_depth(TUM1, 2)
    kw = dict(orb=HAND_ORB, intr=intr, dist=dist, bf=float(TUM1.bf), raw_depth=raw, inv_factor=rs.inv_depth_factor(TUM1))
    want = oracle_front(ob, frames, **kw)
    got = device_front(gpu_lib, frames, **kw)
    outside = assert_front(ob, got, want, True)
    image = (0.0, 640.0, 0.0, 480.0)
    moved = [float(np.abs(u["x"] - k["x"]).max()) for u, (k, _) in zip(want["un"], want["frames"])]
    print(name, dist, want["bounds"], "outside the grid", outside, "largest shift", moved)
    if name == "k1_zero":
        assert np.count_nonzero(dist) == 3 and want["bounds"] == image and max(moved) == 0.0
    else:
        assert min(moved) > 0.5
    if name in ("give_up", "len2", "len3"):
        # the corners give up (TUM1's k2 without its k3 turns 1 + k1 r^2 + k2 r^4 negative there too): the bounds are the corners put
        # through K^-1 and K, the image within rounding; keypoints nearer the centre do not give up, and some land outside the grid
        assert np.allclose(want["bounds"], image, atol=1e-3) and min(outside) >= 5
    if name in ("len1", "pincushion"):
        assert want["bounds"][0] > 0 and want["bounds"][1] < 640 and want["bounds"][2] > 0 and want["bounds"][3] < 480
    if name == "pincushion":
        assert outside[0] >= 10
