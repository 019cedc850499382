"""tests/fmat_restatement.py -- cv::findFundamentalMat(p1, p2, FM_RANSAC, threshold, confidence) as amos-slam_amd/csrc/amos_fmat_core.h
restates it (OpenCV 4.5's classic RANSACPointSetRegistrator + FMEstimatorCallback, written from memory of the published source:
parity with OpenCV unpinned), in Python floats -- IEEE doubles without fused multiply-add, the same operations in the same order.
TEST INFRASTRUCTURE ONLY: the GPU tests hold amos_fmat_ransac_device to it bit for bit.  The scoring of every model over every point is
numpy (elementwise float64, one rounding per operation, the order of the kernel)."""
import math

import numpy as np

MODEL_POINTS = 7
MAX_ATTEMPTS = 10000
REDRAW_CAP = 1 << 20
BISECT = 160
DBL_EPSILON = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
FLT_EPSILON = 1.1920928955078125e-07
LN2 = 0.6931471805599453
SQRT_HALF = 0.7071067811865476
PAIRS = [(j, k) for j in range(6) for k in range(j)]  # haveCollinearPoints' (j, k) order for the last point i = 6


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(a):
    return math.sqrt(a) if a >= 0 else math.nan


def _abs(a):
    return -a if a < 0 else a


class Rng:
    """cv::RNG: state = (uint32)state * 4164903690 + (state >> 32); next() = low 32 bits."""

    def __init__(self, state=(1 << 64) - 1):
        self.s = state

    def next(self):
        self.s = ((self.s & 0xFFFFFFFF) * 4164903690 + (self.s >> 32)) & ((1 << 64) - 1)
        return self.s & 0xFFFFFFFF


def collinear3(xj, yj, xk, yk, xi, yi):
    f32 = np.float32
    dx1, dy1 = float(f32(xj) - f32(xi)), float(f32(yj) - f32(yi))
    dx2, dy2 = float(f32(xk) - f32(xi)), float(f32(yk) - f32(yi))
    return _abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (((_abs(dx1) + _abs(dy1)) + _abs(dx2)) + _abs(dy2))


def have_collinear(xs, ys):
    return any(collinear3(xs[j], ys[j], xs[k], ys[k], xs[6], ys[6]) for j, k in PAIRS)


def cubic_at(a1, a2, a3, x):
    return ((x + a1) * x + a2) * x + a3


def bisect(a1, a2, a3, lo, hi, increasing):
    for _ in range(BISECT):
        mid = lo * 0.5 + hi * 0.5
        if not (lo < mid < hi):
            break
        if (cubic_at(a1, a2, a3, mid) > 0) == increasing:
            hi = mid
        else:
            lo = mid
    return lo * 0.5 + hi * 0.5


def solve_cubic(c):
    """cv::solveCubic's case split for c0 x^3 + c1 x^2 + c2 x + c3 -> (count, roots)."""
    a0, a1, a2, a3 = c
    if a0 == 0:
        if a1 == 0:
            if a2 == 0:
                return (-1 if a3 == 0 else 0), []
            return 1, [_div(-a3, a2)]
        d = a2 * a2 - (4.0 * a1) * a3
        if not d >= 0:
            return 0, []
        d = _sqrt(d)
        q1, q2 = (-a2 + d) * 0.5, (a2 + d) * -0.5
        if _abs(q1) > _abs(q2):
            r = [_div(q1, a1), _div(a3, q1)]
        else:
            r = [_div(q2, a1), _div(a3, q2)]
        return (2 if d > 0 else 1), r
    a0 = _div(1.0, a0)
    a1, a2, a3 = a1 * a0, a2 * a0, a3 * a0
    if not (a1 - a1 == 0 and a2 - a2 == 0 and a3 - a3 == 0):
        return 0, []
    Q = (a1 * a1 - 3.0 * a2) * (1.0 / 9)
    d = (((a1 * a1) * (a2 * a2 - (4.0 * a1) * a3) + (2.0 * a2) * ((9.0 * a1) * a3 - (2.0 * a2) * a2)) - (27.0 * a3) * a3) * (1.0 / 108)
    B = _abs(a1)
    if _abs(a2) > B:
        B = _abs(a2)
    if _abs(a3) > B:
        B = _abs(a3)
    B = B + 1.0
    if d > 0 and Q > 0:
        sq, m = _sqrt(Q), _div(-a1, 3.0)
        m1, m2 = m - sq, m + sq
        return 3, [bisect(a1, a2, a3, -B, m1, True), bisect(a1, a2, a3, m1, m2, False), bisect(a1, a2, a3, m2, B, True)]
    return 1, [bisect(a1, a2, a3, -B, B, True)]


def run7point(p1, p2):
    """run7Point on 7 correspondences (float32 [7][2] each) -> list of F (9 floats each, row-major)."""
    a = []
    for i in range(7):
        x0, y0, x1, y1 = float(p1[i][0]), float(p1[i][1]), float(p2[i][0]), float(p2[i][1])
        a.append([x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, 1.0])
    beta = [0.0] * 7
    for k in range(7):
        nrm2 = 0.0
        for r in range(k, 9):
            nrm2 = nrm2 + a[k][r] * a[k][r]
        if nrm2 == 0.0:
            continue
        nrm = _sqrt(nrm2)
        a[k][k] = a[k][k] + nrm if a[k][k] >= 0 else a[k][k] - nrm
        vtv = 0.0
        for r in range(k, 9):
            vtv = vtv + a[k][r] * a[k][r]
        beta[k] = _div(2.0, vtv)
        for c in range(k + 1, 7):
            w = 0.0
            for r in range(k, 9):
                w = w + a[k][r] * a[c][r]
            w = w * beta[k]
            for r in range(k, 9):
                a[c][r] = a[c][r] - w * a[k][r]
    f1 = [1.0 if r == 7 else 0.0 for r in range(9)]
    f2 = [1.0 if r == 8 else 0.0 for r in range(9)]
    for k in range(6, -1, -1):
        if beta[k] == 0.0:
            continue
        w1 = w2 = 0.0
        for r in range(k, 9):
            w1 = w1 + a[k][r] * f1[r]
            w2 = w2 + a[k][r] * f2[r]
        w1, w2 = w1 * beta[k], w2 * beta[k]
        for r in range(k, 9):
            f1[r] = f1[r] - w1 * a[k][r]
            f2[r] = f2[r] - w2 * a[k][r]
    f1 = [f1[i] - f2[i] for i in range(9)]

    def m2(p, q, r, s):
        return p * q - r * s
    t0, t1, t2 = m2(f2[4], f2[8], f2[5], f2[7]), m2(f2[3], f2[8], f2[5], f2[6]), m2(f2[3], f2[7], f2[4], f2[6])
    c3 = (f2[0] * t0 - f2[1] * t1) + f2[2] * t2
    c2 = ((((((((f1[0] * t0 - f1[1] * t1) + f1[2] * t2) - f1[3] * m2(f2[1], f2[8], f2[2], f2[7])) + f1[4] * m2(f2[0], f2[8], f2[2], f2[6]))
             - f1[5] * m2(f2[0], f2[7], f2[1], f2[6])) + f1[6] * m2(f2[1], f2[5], f2[2], f2[4])) - f1[7] * m2(f2[0], f2[5], f2[2], f2[3]))
          + f1[8] * m2(f2[0], f2[4], f2[1], f2[3]))
    t0, t1, t2 = m2(f1[4], f1[8], f1[5], f1[7]), m2(f1[3], f1[8], f1[5], f1[6]), m2(f1[3], f1[7], f1[4], f1[6])
    c1 = ((((((((f2[0] * t0 - f2[1] * t1) + f2[2] * t2) - f2[3] * m2(f1[1], f1[8], f1[2], f1[7])) + f2[4] * m2(f1[0], f1[8], f1[2], f1[6]))
             - f2[5] * m2(f1[0], f1[7], f1[1], f1[6])) + f2[6] * m2(f1[1], f1[5], f1[2], f1[4])) - f2[7] * m2(f1[0], f1[5], f1[2], f1[3]))
          + f2[8] * m2(f1[0], f1[4], f1[1], f1[3]))
    c0 = (f1[0] * t0 - f1[1] * t1) + f1[2] * t2
    n, r = solve_cubic((c0, c1, c2, c3))
    if n < 1 or n > 3:
        return []
    out = []
    for k in range(n):
        lam, mu = r[k], 1.0
        s = f1[8] * r[k] + f2[8]
        F = [0.0] * 9
        if _abs(s) > DBL_EPSILON:
            mu = _div(1.0, s)
            lam = lam * mu
            F[8] = 1.0
        for i in range(8):
            F[i] = f1[i] * lam + f2[i] * mu
        out.append(F)
    return out


def log_(x):
    m, e = math.frexp(x)
    if m < SQRT_HALF:
        m, e = m * 2.0, e - 1
    s = _div(m - 1.0, m + 1.0)
    z = s * s
    acc = 1.0 / 23
    for k in (21, 19, 17, 15, 13, 11, 9, 7, 5, 3):
        acc = acc * z + 1.0 / k
    acc = acc * z + 1.0
    return float(e) * LN2 + (2.0 * s) * acc


def round_even(x):
    f = math.floor(x)
    d = x - f
    r = int(f)
    if d > 0.5 or (d == 0.5 and (r & 1)):
        r += 1
    return r


def update_num_iters(p, ep, max_iters):
    """RANSACUpdateNumIters(p, ep, 7, max_iters)."""
    p = 0.0 if p < 0 else (1.0 if p > 1 else p)
    ep = 0.0 if ep < 0 else (1.0 if ep > 1 else ep)
    num = 1.0 - p
    if num < DBL_MIN:
        num = DBL_MIN
    q = 1.0 - ep
    q2 = q * q
    q3 = q2 * q
    q6 = q3 * q3
    q7 = q6 * q
    denom = 1.0 - q7
    if denom < DBL_MIN:
        return 0
    num, denom = log_(num), log_(denom)
    return max_iters if (denom >= 0 or -num >= float(max_iters) * -denom) else round_even(_div(num, denom))


def errors(F, p1, p2):
    """FMEstimatorCallback::computeError for every correspondence: float32 of std::max(d1^2 s1, d2^2 s2) (std::max: a < b ? b : a)."""
    F = [float(v) for v in np.asarray(F, np.float64).reshape(9)]
    x1, y1 = p1[:, 0].astype(np.float64), p1[:, 1].astype(np.float64)
    x2, y2 = p2[:, 0].astype(np.float64), p2[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        a = (F[0] * x1 + F[1] * y1) + F[2]
        b = (F[3] * x1 + F[4] * y1) + F[5]
        c = (F[6] * x1 + F[7] * y1) + F[8]
        s2 = 1.0 / (a * a + b * b)
        d2 = (x2 * a + y2 * b) + c
        a = (F[0] * x2 + F[3] * y2) + F[6]
        b = (F[1] * x2 + F[4] * y2) + F[7]
        c = (F[2] * x2 + F[5] * y2) + F[8]
        s1 = 1.0 / (a * a + b * b)
        d1 = (x1 * a + y1 * b) + c
        e1, e2 = (d1 * d1) * s1, (d2 * d2) * s2
        return np.where(e1 < e2, e2, e1).astype(np.float32)


def get_subset(rng, n, p1, p2):
    """getSubset(..., maxAttempts = 10000) + FMEstimatorCallback::checkSubset -> (indices or None, cap hit)."""
    for _ in range(MAX_ATTEMPTS):
        idx = []
        for i in range(7):
            draws = 0
            while True:
                v = rng.next() % n
                draws += 1
                if v not in idx:
                    break
                if draws >= REDRAW_CAP:
                    return None, True
            idx.append(v)
        s1, s2 = p1[idx], p2[idx]
        if not have_collinear(s1[:, 0], s1[:, 1]) and not have_collinear(s2[:, 0], s2[:, 1]):
            return idx, False
    return None, False


def find_fundamental_ransac(p1, p2, threshold=0.1, confidence=0.99, max_iters=1000):
    """-> (F [9] float64, mask [n] uint8, status (result, inliers, iterations, points)) exactly as amos_fmat_ransac_device computes them
    for one problem whose selected points are p1, p2 (float32 [n][2])."""
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    n = len(p1)
    zero = (np.zeros(9), np.zeros(n, np.uint8))
    if n < 15:
        return zero[0], zero[1], (0 if n < 7 else -1, 0, 0, n)
    thr2 = np.float32(threshold * threshold)
    rng = Rng()
    niters, it, max_good, best = max_iters, 0, 0, None
    while it < niters:
        idx, cap = get_subset(rng, n, p1, p2)
        if cap:
            return zero[0], zero[1], (-2, 0, it, n)
        if idx is None:
            if it == 0:
                return zero[0], zero[1], (0, 0, 0, n)
            break
        for F in run7point(p1[idx], p2[idx]):
            good = int((errors(F, p1, p2) <= thr2).sum())
            if good > max(max_good, MODEL_POINTS - 1):
                best, max_good = F, good
                niters = update_num_iters(confidence, _div(float(n - good), float(n)), niters)
        it += 1
    if max_good <= 0:
        return zero[0], zero[1], (0, 0, it, n)
    F = np.array(best, np.float64)
    return F, (errors(F, p1, p2) <= thr2).astype(np.uint8), (1, max_good, it, n)


def two_view(rng, n, outlier_frac=0.0, noise=0.0, K=None, R=None, t=None):
    """A synthetic two-view scene: random 3-D points in front of both cameras, float32-rounded projections, gross outliers in the second
    view.  Returns (p1, p2, true F normalised to F[8] = 1, inlier flags)."""
    K = np.array([[535.4, 0, 320.1], [0, 539.2, 247.6], [0, 0, 1]]) if K is None else K
    if R is None:
        ax, ay, az = 0.02, -0.03, 0.01
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        R = Rz @ Ry @ Rx
    t = np.array([0.2, 0.05, -0.03]) if t is None else t
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 8, n)]
    x1 = X @ K.T
    X2 = X @ R.T + t
    x2 = X2 @ K.T
    p1 = (x1[:, :2] / x1[:, 2:]).astype(np.float32)
    p2 = (x2[:, :2] / x2[:, 2:] + (rng.normal(0, noise, (n, 2)) if noise else 0)).astype(np.float32)
    inl = np.ones(n, bool)
    k = int(round(outlier_frac * n))
    if k:
        o = rng.choice(n, k, replace=False)
        p2[o] += (rng.uniform(20, 80, (k, 2)) * rng.choice([-1, 1], (k, 2))).astype(np.float32)
        inl[o] = False
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return p1, p2, (F / F[2, 2]).reshape(9), inl
