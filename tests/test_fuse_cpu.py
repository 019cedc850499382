"""The restatement of ORBmatcher::Fuse (tests/fuse_restatement.py) on the CPU: it must equal the pre-filter of tests/adaptor_prefilter.py fed to
the oracle's orc_window_search on the scene the GPU test uses, and that scene must hold every case the GPU test relies on -- so a pass on the GPU
means something.  Also the exports and the size of amos_fuse_camera."""
import ctypes
import re

import numpy as np
import pytest

import fuse_restatement as fr
import host_binding as hb


@pytest.fixture(scope="module")
def sc():
    return fr.scene()


@pytest.fixture(scope="module")
def results(sc):
    out = {}
    for mode in (fr.LOCAL, fr.SIM3):
        for with_right in (True, False):
            infos = []
            out[mode, with_right] = (fr.fuse(sc["kfs"], sc["points"], sc["pairs"], sc["skip"], sc["n_out"], sc["sf"], sc["inv_sigma2"], sc["bounds"],
                                             mode, with_right=with_right, infos=infos), infos)
    return out


@pytest.mark.parametrize("mode", [fr.LOCAL, fr.SIM3])
@pytest.mark.parametrize("with_right", [True, False])
def test_restatement_equals_prefilter_plus_oracle(ob, sc, results, mode, with_right):
    got, _ = results[mode, with_right]
    for p, (frame, first, count, off, cam) in enumerate(sc["pairs"]):
        best, accepted = fr.oracle_pair(hb, sc["kfs"][frame], sc["points"][first:first + count], sc["skip"][off:off + count], cam, sc["sf"],
                                        sc["inv_sigma2"], sc["bounds"], mode, with_right)
        print(f"mode {mode} right {with_right} pair {p}: {count} points, in view {got['stats'][p][0]}, accepted {got['stats'][p][1]} / {accepted}")
        assert np.array_equal(got["best_idx"][off:off + count], best), p
        assert got["stats"][p][1] == accepted, p


def test_scene_holds_the_cases(sc, results):
    got, infos = results[fr.LOCAL, True]
    counts = [c for _, _, c, _, _ in sc["pairs"]]
    assert sorted(counts) == [0, 1, 31, 33, 257, 257, 700]
    assert sc["pairs"][4][1:3] == sc["pairs"][6][1:3] and sc["pairs"][4][3] != sc["pairs"][6][3]   # one range, two pairs
    assert [len(k[0]) for k in sc["kfs"]] == [0, 37, 300, 600]
    for p, (frame, first, count, off, cam) in enumerate(sc["pairs"]):
        if count >= 31:
            assert got["stats"][p][1] >= 10, (p, got["stats"][p])
    assert sc["pairs"][1][0] == 0 and tuple(got["stats"][1]) == (1, 0)                                      # the pair on the empty keyframe
    a, b = sc["pairs"][4][3], sc["pairs"][6][3]
    assert not np.array_equal(sc["skip"][a:a + 257], sc["skip"][b:b + 257]) and sc["skip"][a:a + 257].any() and sc["skip"][b:b + 257].any()
    owned = np.zeros(sc["n_out"], bool)
    for _, _, count, off, _ in sc["pairs"]:
        owned[off:off + count] = True
    for name in fr.REASONS:                                                                        # every exit rejects a point
        assert (got["reason"][owned] == fr.REASONS[name]).sum() >= 1, name
    # the hand points: one per outcome, the boundary values exactly on the boundary
    off, want = sc["hand"]
    assert np.array_equal(got["reason"][off:off + len(want)], want)
    first = sc["pairs"][5][1]
    pts = sc["points"][first:first + len(want)]
    q = got["query"][off:off + len(want)]
    assert q["u"][7] == np.float32(fr.BOUNDS[0]) and q["v"][9] == np.float32(fr.BOUNDS[2])         # u == min_x, v == min_y: in
    assert np.float32(512) * np.float32(pts["pos"][6][0] * np.float32(0.5)) + np.float32(250) == np.float32(fr.BOUNDS[1])  # u == max_x: out
    # windows: clipped at each border, wider than eight grid columns, a single cell.  (A window WHOLLY outside the grid cannot follow the
    # pre-filter: KeyFrame::IsInImage and the grid share their bounds, so min_x <= u < max_x and r > 0 always leave a column inside.)
    iv = got["in_view"] == 1
    r = np.zeros(sc["n_out"], np.float32)
    for _, _, count, off, cam in sc["pairs"]:
        r[off:off + count] = cam["th"] * sc["sf"][got["query"]["level"][off:off + count]]
    u, v = got["query"]["u"], got["query"]["v"]
    assert (iv & (u - r < fr.BOUNDS[0])).any() and (iv & (u + r > fr.BOUNDS[1])).any()
    assert (iv & (v - r < fr.BOUNDS[2])).any() and (iv & (v + r > fr.BOUNDS[3])).any()
    assert max(i["columns"] for _, _, i in infos) > 8 and min(i["cells"] for _, _, i in infos if i["cells"]) == 1
    # levels, both kinds of keyframe feature, the chi-square constants, ties, the threshold
    levels = got["query"]["level"][iv]
    assert (levels == 0).any() and (levels == len(sc["sf"]) - 1).any()
    for kps, desc, ur in sc["kfs"][1:]:
        assert (ur >= 0).any() and (ur < 0).any()
    lost = [k for _, _, i in infos for k in i["chi_lost"]]
    assert lost.count(7.8) >= 1 and lost.count(5.99) >= 1, lost
    ties = [(p, i) for p, i, info in infos if info["tie"]]
    assert len(ties) >= 3, ties
    t0, n_twins = sc["twins"]
    n600 = 600
    assert np.array_equal(got["best_idx"][t0:t0 + n_twins], n600 - n_twins + np.arange(n_twins))    # the LATER feature: first in x-major order
    assert got["best_dist"][t0 + n_twins] == 50 and got["best_idx"][t0 + n_twins] >= 0
    assert got["best_dist"][t0 + n_twins + 1] == 51 and got["best_idx"][t0 + n_twins + 1] == -1
    # the loop-closing mode accepts what the chi-square gate rejected, and a monocular call takes the 5.99 branch everywhere
    sim, _ = results[fr.SIM3, True]
    mono, _ = results[fr.LOCAL, False]
    assert (sim["query"]["ur"] == 0).all() and not np.array_equal(sim["best_idx"], got["best_idx"])
    assert not np.array_equal(mono["best_idx"], got["best_idx"])
    # PredictScale: no ratio within 1e-4 (relative) of a table entry, where the table form and the logf form may differ
    for _, first, count, off, cam in sc["pairs"]:
        pts = sc["points"][first:first + count]
        PO = (pts["pos"] - cam["Ow"]).astype(np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            ratio = pts["max_distance"] / np.sqrt((PO * PO).sum(1)).astype(np.float32)
        sel = got["in_view"][off:off + count] == 1
        rel = np.abs(ratio[sel, None] / sc["sf"][None, :] - 1)
        assert rel.size == 0 or rel.min() > 1e-4


def test_exports_and_camera_size(pkg):
    lib = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("amos_match_fuse_batch_device", "amos_match_fuse"):
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "amos_frontend.h")).read()
    body = re.search(r"typedef struct amos_fuse_camera \{(.*?)\} amos_fuse_camera;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    floats = 0
    for decl in re.findall(r"float ([^;]+);", body):
        for name in decl.split(","):
            m = re.search(r"\[(\d+)\]", name)
            floats += int(m.group(1)) if m else 1
    assert 4 * floats == ctypes.sizeof(pkg.FuseCamera) == pkg.FUSE_CAMERA_DTYPE.itemsize == fr.CAMERA.itemsize == pkg.FUSE_CAMERA_BYTES
    source = open(os.path.join(root, "amos-slam_amd", "csrc", "amos_fuse.hip")).read()
    assert f"sizeof(amos_fuse_camera) == {4 * floats}" in source
