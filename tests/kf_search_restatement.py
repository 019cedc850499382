"""ORBmatcher::SearchForTriangulation (ORBmatcher.cc:810-1009, CheckDistEpipolarLine :188-215) and ORBmatcher::SearchByBoW(pKF1, pKF2,
vpMatches12) (:656-799), restated loop by loop in plain Python on the side dicts of bow_search_cases.py (keys, angles, desc, fv, has_point,
and u_right for triangulation).  float32 values are numpy float32 scalars and arrays, so every operation rounds once, in source order.
Independent of the device code: the tests hold the device to it, and test_kf_search_cpu.py holds IT to the CPU oracle.

Beside the reference's result both return what the device forms count: n_queries (keyframe-1 features that reach the candidate loop) and
n_researched (defined per function below)."""
import numpy as np

from bow_restatement import HISTO_LENGTH, TH_LOW, _POP, three_maxima

f32 = np.float32


def _bin(angle1, angle2):
    factor = f32(HISTO_LENGTH) / f32(360.0)
    rot = f32(angle1) - f32(angle2)
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = int(np.floor(float(f32(rot * factor)) + 0.5))  # C round() of a value >= 0: half away from zero
    return 0 if b == HISTO_LENGTH else b


def _prune(match12, hist, nmatches):
    ind = three_maxima([len(h) for h in hist])
    for i in range(HISTO_LENGTH):
        if i in ind:
            continue
        for idx1 in hist[i]:
            match12[idx1] = -1
            nmatches -= 1
    return nmatches


def search_by_bow_kf(k1, k2, nn_ratio, check_orientation):
    """:656-799.  n_researched: the queries whose best or second best over ALL candidates of the node (a good map point, distance below
    256; the first of equal distances each) is already matched at their turn."""
    n1 = len(k1["desc"])
    match12, matched2 = [-1] * n1, set()
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = n_queries = n_researched = n_ties = 0
    nn_ratio = f32(nn_ratio)
    hp1, hp2 = k1.get("has_point"), k2.get("has_point")
    for node in sorted(k1["fv"]):
        if node not in k2["fv"]:
            continue
        lst2 = k2["fv"][node]
        for idx1 in k1["fv"][node]:
            if hp1 is not None and not hp1[idx1]:
                continue
            n_queries += 1
            dists = _POP[np.bitwise_xor(k2["desc"][lst2], k1["desc"][idx1][None, :])].sum(1).tolist()
            best1, best_idx, best2 = 256, -1, 256
            cands = []
            for idx2, dist in zip(lst2, dists):
                if hp2 is not None and not hp2[idx2]:
                    continue
                cands.append((dist, idx2))
                if idx2 in matched2:
                    continue
                if dist < best1:
                    best2, best1, best_idx = best1, dist, idx2
                elif dist < best2:
                    best2 = dist
            top = sorted((c for c in cands if c[0] < 256), key=lambda c: c[0])[:2]  # stable: the first of equal distances
            if any(c[1] in matched2 for c in top):
                n_researched += 1
            if best1 < TH_LOW and f32(best1) < nn_ratio * f32(best2):
                match12[idx1] = best_idx
                matched2.add(best_idx)
                n_ties += best1 == best2
                if check_orientation:
                    hist[_bin(k1["angles"][idx1], k2["angles"][best_idx])].append(idx1)
                nmatches += 1
    if check_orientation:
        nmatches = _prune(match12, hist, nmatches)
    return np.array(match12, np.int32), {"n_queries": n_queries, "n_matches": nmatches, "n_researched": n_researched, "n_ties": n_ties}


def search_for_triangulation(k1, k2, f12, ex, ey, scale_factors2, level_sigma2_2, only_stereo, check_orientation):
    """:810-1009.  The tests of a candidate that do not depend on what is matched: no map point, stereo under only_stereo, dist <= TH_LOW,
    not near the epipole (both mono), the line test.  n_researched: the queries whose LAST candidate of the smallest distance among those
    passing these tests AND the next one in the same order (smallest distance, then latest) are both matched at their turn.
    epipole_rejected / line_rejected: the candidates the reference's loop, as it runs (running bound and matched features included), drops
    at :899-905 / :907; n_ties: accepted matches with another free passing candidate of the same distance."""
    n1 = len(k1["desc"])
    F = np.asarray(f12, f32).reshape(9)
    ex, ey = f32(ex), f32(ey)
    sf, sg = np.asarray(scale_factors2, f32), np.asarray(level_sigma2_2, f32)
    match12, matched2 = [-1] * n1, set()
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = n_queries = n_researched = n_ep = n_line = n_ties = 0
    hp1, hp2, ur1, ur2 = k1.get("has_point"), k2.get("has_point"), k1.get("u_right"), k2.get("u_right")
    x2a, y2a, oct2a = k2["keys"]["x"].astype(f32), k2["keys"]["y"].astype(f32), k2["keys"]["octave"]
    with np.errstate(all="ignore"):
        for node in sorted(k1["fv"]):
            if node not in k2["fv"]:
                continue
            lst2 = np.asarray(k2["fv"][node], np.int64)
            x2, y2, o2 = x2a[lst2], y2a[lst2], oct2a[lst2]
            stereo2 = (ur2[lst2] >= 0) if ur2 is not None else np.zeros(len(lst2), bool)
            plain = np.ones(len(lst2), bool) if hp2 is None else ~np.asarray(hp2, bool)[lst2]
            if only_stereo:
                plain &= stereo2
            near = ((ex - x2) * (ex - x2) + (ey - y2) * (ey - y2)) < f32(100) * sf[o2]  # :899-905
            for idx1 in k1["fv"][node]:
                if hp1 is not None and hp1[idx1]:
                    continue
                stereo1 = bool(ur1 is not None and ur1[idx1] >= 0)
                if only_stereo and not stereo1:
                    continue
                n_queries += 1
                dists = _POP[np.bitwise_xor(k2["desc"][lst2], k1["desc"][idx1][None, :])].sum(1)
                x1, y1 = f32(k1["keys"]["x"][idx1]), f32(k1["keys"]["y"][idx1])
                a = x1 * F[0] + y1 * F[3] + F[6]  # :191-193
                b = x1 * F[1] + y1 * F[4] + F[7]
                c = x1 * F[2] + y1 * F[5] + F[8]
                num = a * x2 + b * y2 + c
                den = a * a + b * b
                dsqr = num * num / den
                line_ok = (dsqr.astype(np.float64) < 3.84 * sg[o2].astype(np.float64)) if den != 0 else np.zeros(len(lst2), bool)
                at_epipole = near & ~stereo2 if not stereo1 else np.zeros(len(lst2), bool)
                best_dist, best_idx = TH_LOW, -1
                for j in np.nonzero(plain & (dists <= TH_LOW))[0].tolist():  # the reference's loop
                    idx2 = int(lst2[j])
                    if idx2 in matched2 or dists[j] > best_dist:
                        continue
                    if at_epipole[j]:
                        n_ep += 1
                        continue
                    if not line_ok[j]:
                        n_line += 1
                        continue
                    best_idx, best_dist = idx2, int(dists[j])
                passing = np.nonzero(plain & (dists <= TH_LOW) & ~at_epipole & line_ok)[0].tolist()
                order = sorted(passing, key=lambda j: (int(dists[j]), -j))
                if len(order) >= 2 and int(lst2[order[0]]) in matched2 and int(lst2[order[1]]) in matched2:
                    n_researched += 1
                if best_idx >= 0:
                    n_ties += sum(1 for j in passing if dists[j] == best_dist and int(lst2[j]) not in matched2) >= 2
                    match12[idx1] = best_idx
                    matched2.add(best_idx)
                    nmatches += 1
                    if check_orientation:
                        hist[_bin(k1["angles"][idx1], k2["angles"][best_idx])].append(idx1)
    if check_orientation:
        nmatches = _prune(match12, hist, nmatches)
    return np.array(match12, np.int32), {"n_queries": n_queries, "n_matches": nmatches, "n_researched": n_researched,
                                         "epipole_rejected": n_ep, "line_rejected": n_line, "n_ties": n_ties}
