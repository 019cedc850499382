"""CPU: the steered case table of tests/ransac_steering.py.  (1) The census -- the restatement run with its solvers wrapped -- shows that
every cell the GPU test relies on is filled: each root of run7Point's cubic, each P3P solution index, slots on both sides of the
64-iteration round boundary, a redrawn subset, both ties, a select mask, every refit inlier count.  (2) Every steered winning hypothesis is
checked on its own sample with mpmath at 50 digits, so the table pins models that ARE solutions, not whatever the restatement emits."""
import collections

import mpmath as mp
import numpy as np
import pytest

import fmat_restatement as fr
import pnp_restatement as pr
import ransac_steering as rs

K = rs.K


@pytest.fixture(scope="module")
def rows():
    return rs.table_census()


def _cells(rows, family):
    """cell -> the problems of the family that landed where they were steered (a miss is dropped from its cell)."""
    out = collections.defaultdict(list)
    for fam, cell, p, c, ok in rows:
        if fam == family and ok:
            out[cell].append((p, c))
    return out


def test_table_size_and_miss_share(rows):
    assert len(rows) == rs.TABLE_SIZE <= 320
    built, missed = collections.Counter(), collections.Counter()
    for fam, cell, p, c, ok in rows:
        built[fam] += 1
        missed[fam] += not ok
    print({f: (missed[f], built[f]) for f in built})
    for fam in built:
        assert 8 * missed[fam] <= built[fam], (fam, missed[fam], built[fam])
    assert set(built) == {"fmat_roots", "fmat_geometries", "fmat_slots", "fmat_redraw", "fmat_ties", "select", "p3p", "p3p_dead_slot0", "refit",
                          "pnp_slots", "refit_fallback"}
    # the largest problem: 529 points, 71 iterations
    assert max(len(p["p1"] if p["kind"] == "fmat" else p["obj"]) for _, _, p, _, _ in rows) == 529
    assert max(c["want"][2][2] for _, _, _, c, _ in rows) == 71


def test_every_root_wins_at_slot_0(rows):
    cells = _cells(rows, "fmat_roots")
    for root, nroots in ((0, 3), (1, 3), (2, 3), (0, 1)):
        got = cells[(root, nroots)]
        assert len(got) >= 16, (root, nroots, len(got))
        for p, c in got:
            assert (c["slot"], c["index"], c["count"]) == (0, root, nroots) and c["want"][2] == (1, 24, 1, 24)
            # the returned F is that root's, byte for byte, and no other root's
            assert [np.array(F).tobytes() == c["want"][0].tobytes() for F in c["solutions"]] == [r == root for r in range(nroots)]


def test_every_geometry_and_root(rows):
    cells = _cells(rows, "fmat_geometries")
    for geometry in ("two_view", "coplanar", "near_collinear"):
        for root, nroots in ((0, 3), (1, 3), (2, 3), (0, 1)):
            got = cells[(geometry, root, nroots)]
            assert got, (geometry, root, nroots)
            for p, c in got:
                assert (c["slot"], c["index"], c["count"]) == (0, root, nroots)
                if geometry == "near_collinear":   # the triple passes the sampler, and one float lower it would not
                    a = c["sample"][0]
                    assert not fr.collinear3(a[0][0], a[0][1], a[1][0], a[1][1], a[6][0], a[6][1])
                    assert fr.collinear3(a[0][0], a[0][1], a[1][0], np.nextafter(a[1][1], np.float32(-np.inf)), a[6][0], a[6][1])


def test_slots_on_both_sides_of_the_round_boundary(rows):
    cells = _cells(rows, "fmat_slots")
    for slot in (1, 31, 63, 64, 70):
        for root in range(3):
            got = cells[(slot, root)]
            assert got, (slot, root)
            for p, c in got:
                assert c["want"][2][2] == slot + 1 and (c["slot"], c["index"]) == (slot, root) and len(c["counts"]) == slot + 1
                # it wins by its count alone: every earlier hypothesis has fewer inliers
                assert max(max(x) for x in c["counts"][:slot] if x) < c["counts"][slot][root] == c["want"][2][1]
    cells = _cells(rows, "pnp_slots")
    for slot in (1, 31, 63, 64, 70):
        for m in (4, 5, 6):
            got = cells[(slot, m)]
            assert got, (slot, m)
            for p, c in got:
                assert c["want"][2][:3] == (1, m, slot + 1) and c["slot"] == slot and c["refit"] == 1 and c["refit_count"] == m


def test_redrawn_subset(rows):
    got = _cells(rows, "fmat_redraw")[("redraw",)]
    assert len(got) >= 2
    for p, c in got:
        assert c["attempt0"] >= 1 and c["slot"] == 0
        first = rs.first_draw(24)
        assert sorted(first) != sorted(rs.fmat_subsets(p["p1"], p["p2"], 1)[0][0])
        assert fr.have_collinear(p["p1"][first][:, 0], p["p1"][first][:, 1])


def test_ties(rows):
    cells = _cells(rows, "fmat_ties")
    assert len(cells[("root",)]) >= 2 and len(cells[("slot",)]) >= 2
    for p, c in cells[("root",)]:
        t = p["target"]
        cs = c["counts"][t["slot"]]
        assert cs[0] == cs[t["tie"][1]] == c["want"][2][1] and c["index"] == 0
    for p, c in cells[("slot",)]:
        t = p["target"]
        s2, r2 = t["tie"][1:]
        assert c["counts"][t["slot"]][t["index"]] == c["counts"][s2][r2] == c["want"][2][1]
        assert c["slot"] == t["slot"] < s2 and c["want"][2][2] == s2 + 1


def test_select_mask(rows):
    cells = _cells(rows, "select")
    assert len(cells[("fmat",)]) >= 2 and len(cells[("pnp",)]) >= 2
    for kind in ("fmat", "pnp"):
        for p, c in cells[(kind,)]:
            sel = p["sel"].astype(bool)
            model, mask, st = c["want"]
            assert 0 < (~sel).sum() and st[3] == sel.sum() < len(sel) and not mask[~sel].any() and mask.sum() == st[1]
            raw = np.flatnonzero(mask)
            assert (raw != np.flatnonzero(mask[sel])).any()   # raw positions differ from compacted ones


def test_every_p3p_solution_index(rows):
    cells = _cells(rows, "p3p")
    per_k = collections.Counter()
    for nsol in (1, 2, 3, 4):
        for k in range(nsol):
            got = cells[(nsol, k)]
            assert got, (nsol, k)
            per_k[k] += len(got)
            for p, c in got:
                assert c["want"][2] == (1, 4, 0, 4, 0) and (c["index"], c["count"]) == (k, nsol)
                assert [np.array(s).tobytes() == c["want"][0].tobytes() for s in c["solutions"]] == [j == k for j in range(nsol)]
    assert all(per_k[k] >= 8 for k in range(4)), per_k
    got = _cells(rows, "p3p_dead_slot0")[("dead",)]
    assert got
    for p, c in got:
        assert 0 in c["none_slots"] and c["slot"] == 1 and c["want"][2][:3] == (1, 6, 2)


def test_every_refit_count(rows):
    cells = _cells(rows, "refit")
    for m in (4, 5, 6, 7, 63, 64, 65, 511, 512, 513):
        for planar in (False, True):
            got = cells[(m, planar)]
            assert got, (m, planar)
            for p, c in got:
                assert c["want"][2] == (1, m, 1, m + 16, 1) and c["refit_count"] == m and c["slot"] == 0
                assert np.array(c["model"]).tobytes() != c["want"][0].tobytes()   # the refit, not the P3P model, is returned
                if planar:
                    X = p["obj"].astype(np.float64)
                    assert np.linalg.svd(X - X.mean(0), compute_uv=False)[2] < 1e-5
    got = _cells(rows, "refit_fallback")[("fallback",)]
    assert got   # the bounded search found inputs whose refit is not finite (ransac_steering.py's docstring)
    for p, c in got:
        assert c["refit"] == -1 and np.array(c["model"]).tobytes() == c["want"][0].tobytes() and np.isfinite(c["want"][0]).all()


# ---- every steered winning hypothesis against its own sample, mpmath at 50 digits
def _f_residuals(c):
    a, b = c["sample"]
    F = mp.matrix(3, 3)
    for i in range(9):
        F[i // 3, i % 3] = mp.mpf(c["model"][i])
    top = max(abs(v) for v in F)
    res = max(abs((mp.matrix([[mp.mpf(float(b[i][0])), mp.mpf(float(b[i][1])), 1]]) * F *
                   mp.matrix([mp.mpf(float(a[i][0])), mp.mpf(float(a[i][1])), 1]))[0]) for i in range(7)) / top
    return float(res), float(abs(mp.det(F)) / top ** 3)


def _pose_residuals(c):
    obj, img = c["sample"]
    M = [mp.mpf(v) for v in c["model"]]
    R = mp.matrix(3, 3)
    for i in range(9):
        R[i // 3, i % 3] = M[i]
    rep = mp.mpf(0)
    for i in range(3):
        X = [mp.mpf(float(v)) for v in obj[i]]
        xc, yc, zc = (M[3 * r] * X[0] + M[3 * r + 1] * X[1] + M[3 * r + 2] * X[2] + M[9 + r] for r in range(3))
        rep = max(rep, abs(mp.mpf(K[0]) * xc / zc + mp.mpf(K[2]) - mp.mpf(float(img[i][0]))),
                  abs(mp.mpf(K[1]) * yc / zc + mp.mpf(K[3]) - mp.mpf(float(img[i][1]))))
    return float(rep), float(max(abs(v) for v in (R.T * R - mp.eye(3))))


# test_fmat_cpu.py's bounds for exact correspondences: x2' F x1 / max|F| < 1e-6, |det F| <= 1e-9 max|F|^3
F_GENERIC = (1e-6, 1e-9)
# the near-degenerate families have no bound fixed in advance: 16 times the restatement's worst value on the table's own inputs, which was
# (9.75e-13, 5.64e-22) for the coplanar scenes and (2.31e-13, 5.01e-25) for the near-collinear triples.  These guard the restatement against
# a gross error only; the device is held to it bit for bit
F_DEGENERATE = {"coplanar": (16 * 9.75e-13, 16 * 5.64e-22), "near_collinear": (16 * 2.31e-13, 16 * 5.01e-25)}
# test_pnp_cpu.py bounds a P3P pose on exact float32 correspondences by 2e-5 per element of R | t; a rotation off by 2e-5 moves a pixel
# by fx * 2e-5, the reprojection bound of a sample point here.  R' R - I: test_pnp_cpu.py's 1e-12
POSE_GENERIC = (K[0] * 2e-5, 1e-12)
# the refit-fallback inputs are P3P on collinear object points: measured (7.74e-5 px, 5.21e-16), 16 times that
POSE_DEGENERATE = (16 * 7.74e-5, 16 * 5.21e-16)


def test_steered_hypotheses_are_solutions_of_their_samples(rows):
    mp.mp.dps = 50
    worst = collections.defaultdict(lambda: [0.0, 0.0])
    checked = 0
    for fam, cell, p, c, ok in rows:
        if not ok:
            continue
        if p["kind"] == "fmat":
            key = p["target"]["geometry"]
            got, bound = _f_residuals(c), F_DEGENERATE.get(key, F_GENERIC)
        else:
            key = "collinear object points" if p["target"].get("fallback") else "pose"
            got, bound = _pose_residuals(c), POSE_DEGENERATE if p["target"].get("fallback") else POSE_GENERIC
        worst[key] = [max(a, b) for a, b in zip(worst[key], got)]
        assert got[0] <= bound[0] and got[1] <= bound[1], (fam, cell, got, bound)
        checked += 1
    print(dict(worst))
    assert checked >= rs.TABLE_SIZE * 7 // 8
