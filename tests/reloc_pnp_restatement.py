"""tests/reloc_pnp_restatement.py -- ORB-SLAM2's PnPsolver (src/PnPsolver.cc:120-458: the constructor, SetRansacParameters, iterate,
Refine, CheckInliers and their carried state) as amos-slam_amd/csrc/amos_pnp_core.h and amos_reloc_pnp.hip restate it, in Python floats
-- IEEE doubles without fused multiply-add, the same operations in the same order.  TEST INFRASTRUCTURE ONLY: the host-compiled solver
(tests/host_reloc_pnp) and k_reloc_pnp_iterate are held to it bit for bit.

The solver's compute_pose is the EPnP of pnp_restatement (its helpers, called in epnp's order) with the image point taken as
(double)(float)u directly -- PnPsolver hands pixels to EPnP, there is no undistort round trip.  PARITY WITH THE REFERENCE'S OWN EPnP
(its copy of epnp.cpp over OpenCV's cvSVD / cvInvert / cvSolve) STAYS UNPINNED, exactly as for amos_pnp_core.h: what is held is this
restatement.  Where the reference leaves a value undefined the restatement fixes one:
  the reference's unseeded global rand()    one cv::RNG state per solver (fmat_restatement.Rng), seeded by the caller, carried between calls;
                                            RandomInt(0, s - 1) = (int)(((double)(next() >> 1) / 2147483648.0) * (double)s)
  log / pow of SetRansacParameters          fmat_restatement.log_, pow(eps, 3) = (e * e) * e
  (int)ceil(x) of a NaN or huge quotient    1 - e^3 <= 0 gives nIterations = 1 (what max(1, min(INT_MIN, maxIts)) gives on x86); a log of
                                            the denominator that is not negative, or a quotient >= maxIts, gives maxIts
  more than 4096 correspondences            result code -3, nothing else is read
  bow_match[i] outside the pair's points    the feature is skipped, status bit 1"""
import math

import numpy as np

from fmat_restatement import Rng, _div, log_
from pnp_restatement import (_seqv, betas_for, ccs_of, control_points, eig_order, jacobi_sym, l6x10_rho, r_and_t)

MAX_CORRESPONDENCES = 4096
POINT_SKIP = 1
STATUS_OCTAVE, STATUS_MATCH_INDEX = 1, 2
f32 = np.float32


def epnp_direct(obj, img, fu, fv, uc, vc):
    """PnPsolver::compute_pose on m >= 4 correspondences (float32 [m][3], [m][2]): pnp_restatement.epnp's steps in its order, image
    points as they are -> 12-list R row-major, t (not tested for finiteness: CheckInliers sees it as it is)."""
    m = len(obj)
    pw = obj.astype(np.float64)
    with np.errstate(all="ignore"):
        cw0 = [_div(_seqv(pw[:, j]), float(m)) for j in range(3)]
        d = pw - np.array(cw0)
        S = [[0.0] * 3 for _ in range(3)]
        for r, c in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
            S[r][c] = S[c][r] = _seqv(d[:, r] * d[:, c])
        cw, ci = control_points(S, m, cw0)
        X = pw[:, 0] - cw0[0], pw[:, 1] - cw0[1], pw[:, 2] - cw0[2]
        al = np.zeros((m, 4))
        for j in range(3):
            al[:, 1 + j] = (ci[3 * j] * X[0] + ci[3 * j + 1] * X[1]) + ci[3 * j + 2] * X[2]
        al[:, 0] = ((1.0 - al[:, 1]) - al[:, 2]) - al[:, 3]
        u = img[:, 0].astype(np.float64)
        v = img[:, 1].astype(np.float64)
        M1 = np.zeros((m, 12))
        M2 = np.zeros((m, 12))
        for i in range(4):
            M1[:, 3 * i] = al[:, i] * fu
            M1[:, 3 * i + 2] = al[:, i] * (uc - u)
            M2[:, 3 * i + 1] = al[:, i] * fv
            M2[:, 3 * i + 2] = al[:, i] * (vc - v)
        MtM = np.zeros((12, 12))
        for r in range(12):
            for c in range(r, 12):
                inter = np.empty(2 * m)
                inter[0::2] = M1[:, r] * M1[:, c]
                inter[1::2] = M2[:, r] * M2[:, c]
                MtM[r, c] = MtM[c, r] = _seqv(inter)
        lam, V = jacobi_sym(MtM)
        order = eig_order(lam, False)
        nullv = [[float(V[k, order[i]]) for k in range(12)] for i in range(4)]
        L, rho = l6x10_rho(nullv, cw)
        res = []
        for which in (1, 2, 3):
            betas = betas_for(L, rho, which)
            ccs = ccs_of(betas, nullv)
            pc = np.zeros((m, 3))
            for j in range(3):
                pc[:, j] = ((al[:, 0] * ccs[0][j] + al[:, 1] * ccs[1][j]) + al[:, 2] * ccs[2][j]) + al[:, 3] * ccs[3][j]
            if pc[0, 2] < 0.0:
                pc = -pc
            pc0 = [_div(_seqv(pc[:, j]), float(m)) for j in range(3)]
            pw0 = [_div(_seqv(pw[:, j]), float(m)) for j in range(3)]
            H = [_seqv((pc[:, r] - pc0[r]) * (pw[:, c] - pw0[c])) for r in range(3) for c in range(3)]
            Rt = r_and_t(H, pc0, pw0)
            Xc = ((Rt[0] * pw[:, 0] + Rt[1] * pw[:, 1]) + Rt[2] * pw[:, 2]) + Rt[9]
            Yc = ((Rt[3] * pw[:, 0] + Rt[4] * pw[:, 1]) + Rt[5] * pw[:, 2]) + Rt[10]
            inv_Zc = 1.0 / (((Rt[6] * pw[:, 0] + Rt[7] * pw[:, 1]) + Rt[8] * pw[:, 2]) + Rt[11])
            ue = uc + fu * Xc * inv_Zc
            ve = vc + fv * Yc * inv_Zc
            rep = _div(_seqv(np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))), float(m))
            res.append((rep, Rt))
    N = 0
    if res[1][0] < res[0][0]:
        N = 1
    if res[2][0] < res[N][0]:
        N = 2
    return [float(x) for x in res[N][1]]


def ransac_parameters(N, probability, min_inliers, max_iterations, epsilon):
    """SetRansacParameters(p, minInliers, maxIts, 4, eps, .) for N correspondences -> (minInliers, maxIts, eps as float32)."""
    eps = f32(epsilon)
    scaled = f32(N) * eps
    n_min = int(scaled) if scaled < f32(1073741824.0) else 1073741824
    n_min = max(n_min, min_inliers, 4)
    if N > 0:
        q = f32(n_min) / f32(N)
        if eps < q:
            eps = q
    if n_min == N:
        n_it = 1
    else:
        e = float(eps)
        arg = 1.0 - (e * e) * e
        if not arg > 0:
            n_it = 1
        else:
            num, den = log_(1.0 - probability), log_(arg)
            if not den < 0:
                n_it = max_iterations
            else:
                quot = _div(num, den)
                n_it = max_iterations if quot >= float(max_iterations) else int(math.ceil(quot))
    return n_min, max(1, min(n_it, max_iterations)), eps


def random_int(rng, s):
    """DUtils::Random::RandomInt(0, s - 1) with a 31-bit rand() drawn from the solver's generator."""
    r = rng.next()
    return int((float(r >> 1) / 2147483648.0) * float(s))


def draw4(rng, N):
    """The four draws of one iteration as the device makes them: position randi of slot k is looked up in a substitution table of the
    earlier swaps (position -> the back entry that was moved there) instead of a copied index list."""
    pos, val, idx = [], [], []
    for k in range(4):
        s = N - k
        randi = random_int(rng, s)

        def at(p):
            for q in range(len(pos) - 1, -1, -1):
                if pos[q] == p:
                    return val[q]
            return p
        idx.append(at(randi))
        back = at(s - 1)
        pos.append(randi)
        val.append(back)
    return idx


def check_inliers(Rt, P3D, P2D, max_err, fu, fv, uc, vc):
    """CheckInliers for every correspondence -> bool [N]."""
    M = [float(x) for x in Rt]
    X, Y, Z = (P3D[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        Xc = (((M[0] * X + M[1] * Y) + M[2] * Z) + M[9]).astype(f32)
        Yc = (((M[3] * X + M[4] * Y) + M[5] * Z) + M[10]).astype(f32)
        invZc = (1.0 / (((M[6] * X + M[7] * Y) + M[8] * Z) + M[11])).astype(f32)
        ue = uc + (fu * Xc.astype(np.float64)) * invZc.astype(np.float64)
        ve = vc + (fv * Yc.astype(np.float64)) * invZc.astype(np.float64)
        distX = (P2D[:, 0].astype(np.float64) - ue).astype(f32)
        distY = (P2D[:, 1].astype(np.float64) - ve).astype(f32)
        error2 = distX * distX + distY * distY
        return error2 < max_err


def tcw_of(Rt):
    """R | t in double -> the 12 floats of mTcw's first three rows."""
    return np.array([Rt[0], Rt[1], Rt[2], Rt[9], Rt[3], Rt[4], Rt[5], Rt[10], Rt[6], Rt[7], Rt[8], Rt[11]], np.float64).astype(f32)


class Result:
    """What one iterate() call returns (amos_reloc_pnp_result)."""

    def __init__(self, n_features):
        self.code = 0
        self.Tcw = np.zeros(12, f32)
        self.has_pose = self.no_more = self.refined = 0
        self.n_inliers = 0
        self.n_correspondences = self.min_inliers = self.max_iterations = 0
        self.iterations = self.iterations_call = self.best_inliers = 0
        self.status = 0
        self.inlier = np.zeros(n_features, np.uint8)


class PnPsolver:
    """The constructor reads kps (KP_DTYPE [n]), bow_match (int32 [n]) and points (RELOC_POINT_DTYPE [n_points]); seed is the 64-bit state of
    the solver's generator."""

    def __init__(self, kps, bow_match, points, level_sigma2, K, seed):
        self.n_features = len(kps)
        self.fu, self.fv, self.uc, self.vc = (float(f32(x)) for x in K)
        self.status, self.code = 0, 0
        key, sigma2 = [], []
        for i in range(len(kps)):
            j = int(bow_match[i])
            if j < 0:
                continue
            if j >= len(points):
                self.status |= STATUS_MATCH_INDEX
                continue
            if int(points["flags"][j]) & POINT_SKIP:
                continue
            octave = int(kps["octave"][i])
            if octave < 0 or octave >= len(level_sigma2):
                self.status |= STATUS_OCTAVE
                continue
            key.append(i)
            sigma2.append(f32(level_sigma2[octave]))
        self.N = len(key)
        if self.N > MAX_CORRESPONDENCES:
            self.code = -3
            return
        self.key = np.array(key, np.int64)
        self.sigma2 = np.array(sigma2, f32)
        self.P2D = np.stack([kps["x"][self.key], kps["y"][self.key]], 1).astype(f32) if self.N else np.zeros((0, 2), f32)
        self.P3D = points["pos"][np.asarray(bow_match)[self.key]].astype(f32) if self.N else np.zeros((0, 3), f32)
        self.rng = Rng(seed & ((1 << 64) - 1))
        self.iterations = 0
        self.best_inliers = 0
        self.best_mask = np.zeros(self.N, bool)
        self.best_Tcw = np.zeros(12, f32)
        self.n_solves = self.n_nonfinite = 0
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, epsilon=0.4, th2=5.991):
        if self.code:
            return
        self.min_inliers, self.max_iterations, self.eps = ransac_parameters(self.N, probability, min_inliers, max_iterations, epsilon)
        self.max_err = self.sigma2 * f32(th2)

    def _check(self, Rt):
        return check_inliers(Rt, self.P3D, self.P2D, self.max_err, self.fu, self.fv, self.uc, self.vc)

    def _result(self, Tcw, mask, n, refined, no_more, iterations_call):
        r = Result(self.n_features)
        r.status = self.status
        r.n_correspondences, r.min_inliers, r.max_iterations = self.N, self.min_inliers, self.max_iterations
        r.iterations, r.iterations_call, r.best_inliers = self.iterations, iterations_call, self.best_inliers
        r.no_more = int(no_more)
        r.n_solves = self.n_solves  # EPnP solves so far, Refine's included (not part of the record)
        r.n_nonfinite = self.n_nonfinite  # minimal solves so far whose pose was not finite (not part of the record)
        if Tcw is not None:
            r.has_pose, r.refined, r.n_inliers, r.Tcw = 1, int(refined), int(n), Tcw.copy()
            r.inlier[self.key[mask]] = 1
        return r

    def refine(self):
        idx = np.nonzero(self.best_mask)[0]
        Rt = epnp_direct(self.P3D[idx], self.P2D[idx], self.fu, self.fv, self.uc, self.vc)
        self.n_solves += 1
        mask = self._check(Rt)
        n = int(mask.sum())
        return n > self.min_inliers, tcw_of(Rt), mask, n

    def iterate(self, n_iterations):
        if self.code:
            r = Result(self.n_features)
            r.code, r.n_correspondences, r.status = self.code, self.N, self.status
            return r
        if self.N < self.min_inliers:
            return self._result(None, None, 0, 0, True, 0)
        cur = 0
        while self.iterations < self.max_iterations or cur < n_iterations:
            cur += 1
            self.iterations += 1
            idx = draw4(self.rng, self.N)
            Rt = epnp_direct(self.P3D[idx], self.P2D[idx], self.fu, self.fv, self.uc, self.vc)
            self.n_solves += 1
            mask = self._check(Rt)
            n = int(mask.sum())
            if not all(x - x == 0 for x in Rt):  # a degenerate sample: the pose is not finite and nothing is an inlier
                self.n_nonfinite += 1
                assert n == 0
            if n >= self.min_inliers:
                if n > self.best_inliers:
                    self.best_mask, self.best_inliers, self.best_Tcw = mask, n, tcw_of(Rt)
                ok, Tcw, rmask, rn = self.refine()
                if ok:
                    return self._result(Tcw, rmask, rn, 1, False, cur)
        if self.iterations >= self.max_iterations:
            if self.best_inliers >= self.min_inliers:
                return self._result(self.best_Tcw, self.best_mask, self.best_inliers, 0, True, cur)
            return self._result(None, None, 0, 0, True, cur)
        return self._result(None, None, 0, 0, False, cur)


def match_and_found(result, bow_match, n_points):
    """The loop of Tracking.cc:2704-2713 on a result with a pose: (match [n], found [n_points])."""
    bow_match = np.asarray(bow_match, np.int32)
    match = np.where(result.inlier != 0, bow_match, -1).astype(np.int32)
    found = np.zeros(n_points, np.uint8)
    found[match[match >= 0]] = 1
    return match, found
