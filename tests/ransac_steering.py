"""tests/ransac_steering.py -- inputs STEERED so that a chosen hypothesis of amos_fmat_ransac_device / amos_pnp_ransac_device is the model
the RANSAC returns: a chosen root of run7Point's cubic, a chosen solution of P3P, a chosen slot of a round of 64 drawn-ahead subsets, a
chosen inlier count of the EPnP refit.  TEST INFRASTRUCTURE ONLY, CPU only, built on tests/fmat_restatement.py and tests/pnp_restatement.py:
the kernels are not changed and give no debug output; the tests (test_ransac_steering_cpu.py, test_gpu_ransac_steering.py) reach every
hypothesis through the entry points the earlier tests use.

  steer_fmat    float32 points; the subset of iteration `slot` (fr.get_subset replayed from a fresh fr.Rng()) solved with fr.run7point;
                `extra` other points moved in the second image onto the epipolar lines F_root x1 (their x or y kept), the rest gross
                outliers; expected = fr.find_fundamental_ransac(p1, p2, max_iters = slot + 1)
  steer_p3p4    a 4-point problem (returned without a refit) whose fourth image point is the float32 projection of the fourth object
                point under solution k of pr.p3p_all
  steer_pnp     every point a gross outlier but the four of iteration `slot` (a consistent minimal problem) and m - 4 more, which get
                the float32 projections under that slot's p3p4 model; expected = pr.solve_pnp_ransac(..., max_iters = slot + 1)
  census        the restatement run with run7point / get_subset / p3p4 / p3p_all / errors / epnp wrapped: where the returned model came
                from (slot, root or solution index, root or solution count, the sampler attempt of slot 0, refit status and count).  The
                builders' intent is no evidence: every coverage claim of the tests is asserted from the census, a problem that did not
                land where it was steered is dropped from its cell (and still compared on the device)
  table         the case table both tests share (TABLE_SIZE problems; building it and taking its census -- every expected value of the
                GPU test -- took TABLE_SECONDS on one CPU core when this was written, pure Python)

Not covered, because float32 points do not reach them: cv::solveCubic's a0 == 0 branches and run7Point's F[8] = 0 form (|f1[8] r + f2[8]|
<= DBL_EPSILON).  The refit fallback (status -1: EPnP not finite, the RANSAC's P3P model returned) IS covered: search_refit_fallback finds
it within a handful of tries among inlier sets on one world line, where EPnP's H has rank 1 and R is 0 / 0."""
import contextlib
import functools

import numpy as np

import fmat_restatement as fr
import pnp_restatement as pr

K = pr.K_TUM
W, H = 640.0, 480.0
TABLE_SIZE = 242     # asserted by the CPU test
TABLE_SECONDS = "3 s"
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- fundamental matrix
def fmat_subsets(p1, p2, count):
    """The subsets of iterations 0 .. count - 1 (None from the iteration the sampler fails at) and the sampler attempt each one passed
    checkSubset at (0: the first draw)."""
    rng = fr.Rng()
    out = []
    for _ in range(count):
        state = rng.s
        idx, cap = fr.get_subset(rng, len(p1), p1, p2)
        if idx is None:
            out.append((None, -1))
            break
        out.append((idx, _attempt_of(state, len(p1), idx)))
    return out


def _draw7(rng, n):
    idx = []
    for _ in range(7):
        while True:
            v = rng.next() % n
            if v not in idx:
                break
        idx.append(v)
    return idx


def _attempt_of(state, n, idx):
    rng = fr.Rng(state)
    for attempt in range(fr.MAX_ATTEMPTS):
        if _draw7(rng, n) == idx:
            return attempt
    return -1


def first_draw(n):
    """The seven indices of the very first draw of a problem of n points (before checkSubset)."""
    return _draw7(fr.Rng(), n)


def _two_view_points(rng, n, coplanar):
    if not coplanar:
        p1, p2, _, _ = fr.two_view(rng, n)
        return p1, p2
    # a wall a x + b y + c = Z seen by fr.two_view's cameras: x2 ~ H x1, the 7-point system has a three-dimensional null space
    Kc = np.array([[535.4, 0, 320.1], [0, 539.2, 247.6], [0, 0, 1]])
    R, t = pr.rot(0.02, -0.03, 0.01), np.array([0.2, 0.05, -0.03])
    xy = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n)]
    X = np.c_[xy, 4.0 + 0.3 * xy[:, 0] - 0.2 * xy[:, 1]]
    x1, x2 = X @ Kc.T, (X @ R.T + t) @ Kc.T
    return (x1[:, :2] / x1[:, 2:]).astype(f32), (x2[:, :2] / x2[:, 2:]).astype(f32)


def _uniform(rng, n):
    return np.c_[rng.uniform(0, W, n), rng.uniform(0, H, n)].astype(f32)


def _plant_collinear(p, i, j, k):
    """p[j], p[k] onto a line through p[i], exactly (small integers times a power of two: the cross product is 0)."""
    base = np.floor(p[i]).astype(f32)
    p[i] = base
    p[j] = base + f32([16.0, 8.0])
    p[k] = base + f32([48.0, 24.0])


def _nearly_collinear(p, i, j, k):
    """p[k] on the line p[i] p[j], then its y stepped up float by float until collinear3 (i last, as haveCollinearPoints calls it) just
    fails: the triple sits right above the sampler's threshold."""
    base = np.floor(p[i]).astype(f32)
    p[i] = base
    p[j] = base + f32([16.0, 8.0])
    p[k] = base + f32([48.0, 24.0])
    while fr.collinear3(p[j][0], p[j][1], p[k][0], p[k][1], p[i][0], p[i][1]):
        p[k][1] = np.nextafter(p[k][1], f32(np.inf))


def _onto_line(F, p1, p2, i):
    """p2[i] moved onto the epipolar line F x1[i] keeping its x (or its y where the line is steep), rounded to float32; False when the
    new coordinate leaves [-2000, 3000] (float32 steps grow, and an inlier there says little)."""
    M = np.asarray(F, np.float64).reshape(3, 3)
    a, b, c = M @ np.array([float(p1[i][0]), float(p1[i][1]), 1.0])
    x, y = float(p2[i][0]), float(p2[i][1])
    if abs(b) >= abs(a):
        if b == 0:
            return False
        y = -(a * x + c) / b
    else:
        x = -(b * y + c) / a
    if not (-2000.0 < x < 3000.0 and -2000.0 < y < 3000.0):
        return False
    p2[i] = f32([x, y])
    return True


def steer_fmat(rng, n, slot, root, geometry="uniform", extra=12, nroots=3, tie=None, tries=400):
    """-> problem dict, or None when `tries` draws gave no subset with `nroots` roots.  geometry: "uniform" (random points, every
    correspondence a gross outlier), "two_view" (fr.two_view: the tracker's small inter-frame motion), "coplanar" (a wall),
    "near_collinear" (the subset's points 0, 1, 6 a triple just above collinear3's threshold in the first image), "redraw" (a collinear
    triple planted where the first draw of slot 0 lands: the steered subset is a redrawn one).  tie: None, ("root", r2) -- as many points
    onto root r2's lines as onto `root`'s -- or ("slot", s2, r2) -- as many onto root r2 of the later slot s2 (max_iters = s2 + 1)."""
    last = slot if not (tie and tie[0] == "slot") else tie[1]
    for _ in range(tries):
        if geometry in ("two_view", "coplanar"):
            p1, p2 = _two_view_points(rng, n, geometry == "coplanar")
        else:
            p1, p2 = _uniform(rng, n), _uniform(rng, n)
        if geometry == "redraw":
            d = first_draw(n)
            _plant_collinear(p1, d[6], d[0], d[1])
        subs = fmat_subsets(p1, p2, last + 1)
        if subs[-1][0] is None:
            continue
        idx = subs[slot][0]
        if geometry == "near_collinear":
            _nearly_collinear(p1, idx[6], idx[0], idx[1])
            if fmat_subsets(p1, p2, last + 1) != subs:
                continue
        Fs = fr.run7point(p1[idx], p2[idx])
        if len(Fs) != nroots:
            continue
        plans = [(Fs[root], extra)]
        used = set(idx)
        if tie and tie[0] == "root":
            plans.append((Fs[tie[1]], extra))
        elif tie and tie[0] == "slot":
            idx2 = subs[tie[1]][0]
            F2 = fr.run7point(p1[idx2], p2[idx2])
            if len(F2) <= tie[2]:
                continue
            plans.append((F2[tie[2]], extra))
            used |= set(idx2)
        if geometry in ("two_view", "coplanar"):   # the scene's own points fit its true F: every point not steered becomes an outlier
            keep = sorted(used)
            q = _uniform(rng, n)
            q[keep] = p2[keep]
            p2 = q
        free = [i for i in rng.permutation(n) if i not in used]
        ok = True
        for F, cnt in plans:
            done = 0
            while done < cnt and free:
                done += _onto_line(F, p1, p2, free.pop())
            ok &= done == cnt
        if not ok or fmat_subsets(p1, p2, last + 1) != subs:   # the subsets did not move (p2 enters checkSubset too)
            continue
        return dict(kind="fmat", p1=p1, p2=p2, sel=None, max_iters=last + 1,
                    target=dict(slot=slot, index=root, count=nroots, geometry=geometry, good=7 + extra, tie=tie))
    return None


def with_select(rng, prob, drop=0.35):
    """The compacted problem scattered over raw positions: unselected entries (random points) between the selected ones."""
    n = len(prob["p1"] if prob["kind"] == "fmat" else prob["obj"])
    gaps = rng.random(n) < drop
    raw = int(n + gaps.sum())
    sel = np.ones(raw, np.uint8)
    pos, k = [], 0
    for i in range(n):
        if gaps[i]:
            sel[k] = 0
            k += 1
        pos.append(k)
        k += 1
    out = dict(prob, sel=sel)
    for key, dim in (("p1", 2), ("p2", 2)) if prob["kind"] == "fmat" else (("obj", 3), ("img", 2)):
        a = rng.uniform(0, 400, (raw, dim)).astype(f32)
        a[pos] = prob[key]
        out[key] = a
    return out


# ----------------------------------------------------------------------------------------------------------------------------- PnP
def pnp_subsets(n, count):
    rng = fr.Rng()
    return [pr.get_subset(rng, n) for _ in range(count)]


def project32(Rt, X):
    """The float32 pixel k_pnp_score compares with (pr.errors' arithmetic) of one object point under R | t."""
    M = [float(v) for v in Rt]
    x, y, z = float(X[0]), float(X[1]), float(X[2])
    xc = ((M[0] * x + M[1] * y) + M[2] * z) + M[9]
    yc = ((M[3] * x + M[4] * y) + M[5] * z) + M[10]
    zc = ((M[6] * x + M[7] * y) + M[8] * z) + M[11]
    zc = 1.0 / zc if zc != 0.0 else 1.0
    return f32([f32(xc * zc * K[0] + K[2]), f32(yc * zc * K[1] + K[3])])


def _multi_scene(rng):
    """Four points whose first three see the camera near the axis through their circumcentre: where P3P has three or four solutions far
    more often than for pr.scene's random triangles (2 and 7 subsets of 646)."""
    ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.normal(0, 0.25, 3)
    tri = np.c_[np.cos(ang), np.sin(ang), rng.normal(0, 0.15, 3)] * rng.uniform(0.6, 1.2)
    Xc = np.r_[tri, [[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 0.5)]]]
    Xc = Xc @ pr.rot(*rng.normal(0, 0.25, 3)).T + np.array([rng.normal(0, 0.3), rng.normal(0, 0.3), rng.uniform(1.5, 4.0)])
    R, t = pr.rot(0.05, -0.08, 0.03), np.array([0.1, -0.05, 0.2])
    X = ((Xc - t) @ R).astype(f32)
    Xd = X.astype(np.float64) @ R.T + t
    img = np.c_[K[0] * Xd[:, 0] / Xd[:, 2] + K[2], K[1] * Xd[:, 1] / Xd[:, 2] + K[3]].astype(f32)
    return X, img


def steer_p3p4(rng, k, nsol, tries=3000):
    """-> a 4-point problem whose first three correspondences have `nsol` P3P solutions and whose fourth image point is the float32
    projection of the fourth object point under solution k; None when the bounded search finds no such subset."""
    for _ in range(tries):
        if nsol >= 3:
            obj, img = _multi_scene(rng)
        else:
            obj, img, _, _ = pr.scene(rng, 4)
        with np.errstate(all="ignore"):
            sols, _, _ = pr.p3p_all(obj, img, *K)
        if len(sols) != nsol or not np.isfinite(np.array(sols)).all():
            continue
        img = img.copy()
        img[3] = project32(sols[k], obj[3])
        if not np.isfinite(img[3]).all():
            continue
        return dict(kind="pnp", obj=obj, img=img, sel=None, max_iters=500, target=dict(slot=0, index=k, count=nsol, m=4, direct=True))
    return None


def steer_pnp(rng, n, slot, m, planar=False, dead_slot0=False, tries=200):
    """-> problem dict.  dead_slot0: slot 0's subset is searched (bounded) to have no P3P solution at all, the steered model sits at
    `slot` >= 1."""
    subs = pnp_subsets(n, slot + 1)
    idx = subs[slot]
    for _ in range(tries):
        obj, true_img, _, _ = pr.scene(rng, n, planar=planar)
        img = _uniform(rng, n)
        img[idx] = true_img[idx]
        if dead_slot0:
            with np.errstate(all="ignore"):
                if set(subs[0]) & set(idx) or pr.p3p_all(obj[subs[0]], img[subs[0]], *K)[0]:
                    continue
        Rt = pr.p3p4(obj[idx], img[idx], *K)
        if Rt is None:
            continue
        more = [i for i in rng.permutation(n) if i not in idx and not (dead_slot0 and i in subs[0])][:m - 4]
        for i in more:
            img[i] = project32(Rt, obj[i])
        return dict(kind="pnp", obj=obj, img=img, sel=None, max_iters=slot + 1,
                    target=dict(slot=slot, m=m, planar=planar, direct=False, dead_slot0=dead_slot0))
    return None


def search_refit_fallback(rng, tries=2000):
    """A bounded search for an input whose EPnP refit is not finite (status -1: the RANSAC's own P3P model is returned).  The candidates
    are the degenerate inlier sets a tracker can meet: m inliers drawn on one world line or in one axis-aligned world plane, in
    front of the camera, with the consistent projections steer_pnp gives them.  -> (problem or None, tries used)."""
    for trial in range(tries):
        m = int(rng.choice([4, 5, 8]))
        n = m + 16
        idx = pnp_subsets(n, 1)[0]
        obj, _, _, _ = pr.scene(rng, n)
        R, t = pr.rot(0.05, -0.08, 0.03), np.array([0.1, -0.05, 0.2])
        inl = list(idx) + [i for i in rng.permutation(n) if i not in idx][:m - 4]
        kind = trial % 3
        for j, i in enumerate(inl):
            s = rng.uniform(-1.5, 1.5)
            if kind == 0:      # a line along a world axis
                obj[i] = f32([s, 0.0, 0.0])
            elif kind == 1:    # a line through the origin
                obj[i] = f32([s, 0.5 * s, 0.25 * s])
            else:              # the plane z = 0
                obj[i] = f32([s, rng.uniform(-1, 1), 0.0])
        Xd = obj.astype(np.float64) @ R.T + t + np.array([0, 0, 4.0])
        img = _uniform(rng, n)
        img[inl] = np.c_[K[0] * Xd[inl, 0] / Xd[inl, 2] + K[2], K[1] * Xd[inl, 1] / Xd[inl, 2] + K[3]].astype(f32)
        Rt = pr.p3p4(obj[idx], img[idx], *K)
        if Rt is None:
            continue
        for i in inl[4:]:
            img[i] = project32(Rt, obj[i])
        prob = dict(kind="pnp", obj=obj, img=img, sel=None, max_iters=1, target=dict(slot=0, m=m, fallback=True, direct=False))
        if pr.solve_pnp_ransac(obj, img, *K, max_iters=1)[2][4] == -1:
            return prob, trial + 1
    return None, tries


# -------------------------------------------------------------------------------------------------------------------------- census
@contextlib.contextmanager
def _wrapped(module, name, wrapper):
    orig = getattr(module, name)
    setattr(module, name, functools.partial(wrapper, orig))
    try:
        yield
    finally:
        setattr(module, name, orig)


def want_of(prob):
    """The expected (model, mask over raw positions, status) of one problem: the restatement on the selected points."""
    first, second = (prob["p1"], prob["p2"]) if prob["kind"] == "fmat" else (prob["obj"], prob["img"])
    s = np.ones(len(first), bool) if prob["sel"] is None else prob["sel"].astype(bool)
    if prob["kind"] == "fmat":
        model, m, st = fr.find_fundamental_ransac(first[s], second[s], max_iters=prob["max_iters"])
    else:
        model, m, st = pr.solve_pnp_ransac(first[s], second[s], *K, max_iters=prob["max_iters"])
    mask = np.zeros(len(first), np.uint8)
    mask[s] = m
    return np.asarray(model, np.float64), mask, tuple(int(v) for v in st)


def _census_fmat(prob):
    calls, attempts = [], []

    def rec_run7(orig, a, b):
        out = orig(a, b)
        calls.append((np.array(a), np.array(b), [list(F) for F in out]))
        return out

    def rec_subset(orig, rng, n, p1, p2):
        state = rng.s
        idx, cap = orig(rng, n, p1, p2)
        attempts.append(_attempt_of(state, n, idx) if idx is not None else -1)
        return idx, cap

    with _wrapped(fr, "run7point", rec_run7), _wrapped(fr, "get_subset", rec_subset):
        want = want_of(prob)
    s = np.ones(len(prob["p1"]), bool) if prob["sel"] is None else prob["sel"].astype(bool)
    p1, p2 = prob["p1"][s], prob["p2"][s]
    thr2 = f32(0.1 * 0.1)
    counts = [[int((fr.errors(F, p1, p2) <= thr2).sum()) for F in Fs] for _, _, Fs in calls]
    where = None
    for slot, (_, _, Fs) in enumerate(calls):
        for r, F in enumerate(Fs):
            if where is None and want[2][0] == 1 and np.array(F, np.float64).tobytes() == want[0].tobytes():
                where = (slot, r)
    c = dict(want=want, slot=None, index=None, count=None, attempt0=attempts[0] if attempts else None, counts=counts, refit=None,
             refit_count=None, sample=None, model=None, solutions=None)
    if where:
        slot, r = where
        c.update(slot=slot, index=r, count=len(calls[slot][2]), sample=calls[slot][:2], model=calls[slot][2][r], solutions=calls[slot][2])
    return c


def _census_pnp(prob):
    p3p, alls, scored, refits = [], [], [], []

    def rec_p3p4(orig, obj, img, *k):
        out = orig(obj, img, *k)
        p3p.append((np.array(obj), np.array(img), None if out is None else list(out), alls.pop() if alls else []))
        return out

    def rec_all(orig, obj, img, *k):
        out = orig(obj, img, *k)
        alls.append([list(s) for s in out[0]])
        return out

    def rec_errors(orig, Rt, *a):
        scored.append(np.array(Rt, np.float64))
        return orig(Rt, *a)

    def rec_epnp(orig, obj, img, *k):
        out = orig(obj, img, *k)
        refits.append((len(obj), bool(np.isfinite(np.array(out)).all())))
        return out

    with _wrapped(pr, "p3p4", rec_p3p4), _wrapped(pr, "p3p_all", rec_all), _wrapped(pr, "errors", rec_errors), _wrapped(pr, "epnp", rec_epnp):
        want = want_of(prob)
    c = dict(want=want, slot=None, index=None, count=None, attempt0=None, counts=None, refit=want[2][4], refit_count=None, sample=None,
             model=None, solutions=None, none_slots=[i for i, (_, _, out, _) in enumerate(p3p) if out is None])
    if want[2][0] != 1:
        return c
    n = want[2][3]
    best = want[0] if n == 4 else scored[-1]   # the last model scored is the one whose mask is returned and refitted
    for slot, (obj, img, out, sols) in enumerate(p3p):
        if out is not None and np.array(out, np.float64).tobytes() == best.tobytes():
            ks = [k for k, s in enumerate(sols) if np.array(s, np.float64).tobytes() == best.tobytes()]
            c.update(slot=slot, index=ks[0], count=len(sols), sample=(obj, img), model=out, solutions=sols)
            break
    if refits:
        c.update(refit_count=refits[-1][0])
    return c


def census(problems):
    """-> one dict per problem: want (the restatement's model, mask, status), slot and index (root or P3P solution) of the hypothesis
    that IS the returned model (for a refitted PnP problem: the model that was refitted), count (roots or solutions of that subset),
    attempt0 (the sampler attempt slot 0 passed checkSubset at), counts (fmat: the inlier count of every hypothesis, [slot][root]),
    refit (status[4]) and refit_count (the points EPnP was given), sample / model / solutions of the winning subset."""
    return [_census_fmat(p) if p["kind"] == "fmat" else _census_pnp(p) for p in problems]


def landed(prob, c):
    """Did the problem land where it was steered?  Read from the census alone."""
    t, st = prob["target"], c["want"][2]
    if st[0] != 1 or c["slot"] != t["slot"]:
        return False
    if prob["kind"] == "fmat":
        if (c["index"], c["count"]) != (t["index"], t["count"]) or st[1] != t["good"] or st[2] != prob["max_iters"]:
            return False
        if t["geometry"] == "redraw" and not c["attempt0"] >= 1:
            return False
        if t["tie"] and t["tie"][0] == "root":   # both roots reach the winning count, nothing beats it, the earlier root is returned
            cs = c["counts"][t["slot"]]
            return cs[t["index"]] == cs[t["tie"][1]] == max(max(x) for x in c["counts"] if x) and t["index"] < t["tie"][1]
        if t["tie"] and t["tie"][0] == "slot":
            return (c["counts"][t["slot"]][t["index"]] == c["counts"][t["tie"][1]][t["tie"][2]] == max(max(x) for x in c["counts"] if x)
                    and t["slot"] < t["tie"][1] and len(c["counts"]) == t["tie"][1] + 1)
        return True
    if t.get("direct"):
        return st == (1, 4, 0, 4, 0) and (c["index"], c["count"]) == (t["index"], t["count"])
    if st[1] != t["m"] or st[2] != prob["max_iters"] or c["refit_count"] != t["m"]:
        return False
    if t.get("dead_slot0") and 0 not in c["none_slots"]:
        return False
    return c["refit"] == (-1 if t.get("fallback") else 1)


# --------------------------------------------------------------------------------------------------------------------------- table
F_SLOTS = (1, 31, 63, 64, 70)
REFIT_M = (4, 5, 6, 7, 63, 64, 65, 511, 512, 513)
PNP_SLOTS = (1, 31, 63, 64, 70)


@functools.lru_cache(maxsize=None)
def table():
    """-> list of (family, cell, problem).  family names a case family of the tests (one GPU test each), cell the coverage cell inside
    it.  Deterministic: every builder draws from its own seeded generator."""
    out = []

    def add(family, cell, prob):
        if prob is not None:
            out.append((family, cell, prob))

    def gen(*key):
        return np.random.default_rng(list(key))
    # roots at slot 0: n = 24, every other point steered
    for root, nroots in ((0, 3), (1, 3), (2, 3), (0, 1)):
        for i in range(16):
            add("fmat_roots", (root, nroots), steer_fmat(gen(1, root, nroots, i), 24, 0, root, "uniform", 17, nroots))
    for g, geometry in enumerate(("two_view", "coplanar", "near_collinear")):
        for root, nroots in ((0, 3), (1, 3), (2, 3), (0, 1)):
            for i in range(2):
                add("fmat_geometries", (geometry, root, nroots), steer_fmat(gen(2, g, root, nroots, i), 24, 0, root, geometry, 17, nroots))
    for slot in F_SLOTS:
        for root in range(3):
            for i in range(2):
                add("fmat_slots", (slot, root), steer_fmat(gen(3, slot, root, i), 200, slot, root, "uniform", 12))
    for i in range(4):
        add("fmat_redraw", ("redraw",), steer_fmat(gen(4, i), 24, 0, i % 3, "redraw", 17))
    for i in range(4):
        add("fmat_ties", ("root",), steer_fmat(gen(5, i), 200, i % 2, 0, "uniform", 10, tie=("root", 1 + i % 2)))
        add("fmat_ties", ("slot",), steer_fmat(gen(6, i), 200, 1 + i, i % 3, "uniform", 10, tie=("slot", 3 + 2 * i, (i + 1) % 3)))
    for i in range(4):
        p = steer_fmat(gen(7, i), 200 if i % 2 else 24, i % 2, i % 3, "uniform", 12 if i % 2 else 17)
        add("select", ("fmat",), with_select(gen(8, i), p) if p else None)
        p = steer_pnp(gen(9, i), 40, i % 2, 5 + i)
        add("select", ("pnp",), with_select(gen(10, i), p) if p else None)
    # P3P: every (solution count, k)
    for nsol, reps in ((1, 2), (2, 2), (3, 2), (4, 8)):
        for k in range(nsol):
            for i in range(reps):
                add("p3p", (nsol, k), steer_p3p4(gen(11, nsol, k, i), k, nsol))
    for i in range(2):
        add("p3p_dead_slot0", ("dead",), steer_pnp(gen(12, i), 40, 1, 6, dead_slot0=True))
    for m in REFIT_M:
        for planar in (False, True):
            for i in range(2):
                add("refit", (m, planar), steer_pnp(gen(13, m, int(planar), i), m + 16, 0, m, planar))
    for slot in PNP_SLOTS:
        for m in (4, 5, 6):
            add("pnp_slots", (slot, m), steer_pnp(gen(14, slot, m), 80, slot, m))
    for i in range(3):
        add("refit_fallback", ("fallback",), search_refit_fallback(gen(15, i))[0])
    return out


@functools.lru_cache(maxsize=None)
def table_census():
    """-> list of (family, cell, problem, census, landed) for the whole table: computed once, shared by every test."""
    t = table()
    return [(fam, cell, p, c, landed(p, c)) for (fam, cell, p), c in zip(t, census([p for _, _, p in t]))]
