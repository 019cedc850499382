"""Optimizer::PoseOptimization as amos-slam_amd/csrc/amos_pose_core.h states it, in Python floats and numpy, bit for bit: the same
operations in the same order (every numpy ufunc used here is one correctly rounded IEEE operation per element; nothing is fused).  The
per-edge work is vectorised over the edges; the sums follow strided_partials() + tree_sum() of the header."""
import math

import numpy as np

K_THREADS, K_SUMS, K_ROUNDS, K_ITERATIONS, K_TRIALS = 256, 28, 4, 10, 10
DELTA_MONO, DELTA_STEREO = float(np.float32(math.sqrt(5.991))), float(np.float32(math.sqrt(7.815)))
CHI2_MONO, CHI2_STEREO = np.float32(5.991), np.float32(7.815)
DBL_MAX = 1.7976931348623157e308
TINY = 5.562684646268003e-309
TWO_OVER_PI, TWO_PI = 0.6366197723675814, 6.283185307179586
P1, P2, P3, P4 = 1.5707963267341256, 6.077100506303966e-11, 2.0222662487111665e-21, 8.4784276603689e-32
REDUCE_BIG = 65536.0
STATUS_OCTAVE, STATUS_MATCH_INDEX = 1, 2
ACT_TRIAL, ACT_ITERATE, ACT_ROUND_END = 0, 1, 2

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CAMERA = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4")])
RESULT = np.dtype([("Rt", "<f8", (12,)), ("Tcw", "<f4", (12,)), ("Ow", "<f4", (3,)), ("n_edges", "<i4"), ("n_inliers", "<i4"),
                   ("n_inliers_with_obs", "<i4"), ("rounds", "<i4"), ("status", "<i4"), ("iterations", "<i4", (4,)), ("trials", "<i4", (4,)),
                   ("lambda", "<f8", (4,)), ("chi2", "<f8", (4,))])
assert CAMERA.itemsize == 68 and RESULT.itemsize == 272


def fmod_(x, y):
    ex, ey = math.frexp(x)[1], math.frexp(y)[1]
    for e in range(ex - ey, -1, -1):
        s = math.ldexp(y, e)
        if x >= s:
            x = x - s
    return x


SIN_COEF = [1.0 / 355687428096000.0, -1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0,
            1.0 / 120.0, -1.0 / 6.0]
COS_COEF = [-1.0 / 6402373705728000.0, 1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0,
            -1.0 / 720.0, 1.0 / 24.0, -1.0 / 2.0]


def sin_cos(theta):
    if theta >= REDUCE_BIG:
        theta = fmod_(theta, TWO_PI)
    if theta != theta or theta == math.inf:  # (inf - inf in the reduction: NaN, as in the header)
        return math.nan, math.nan
    k = float(math.floor(theta * TWO_OVER_PI + 0.5))
    r = (((theta - k * P1) - k * P2) - k * P3) - k * P4
    z = r * r
    ps = SIN_COEF[0]
    for c in SIN_COEF[1:]:
        ps = ps * z + c
    pc = COS_COEF[0]
    for c in COS_COEF[1:]:
        pc = pc * z + c
    sr, cr = r + r * (z * ps), 1.0 + z * pc
    n = int(k - 4.0 * math.floor(k * 0.25))
    return ((sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr))[n]


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def mat3_mul(A, B):
    return [dot3(A[i * 3], A[i * 3 + 1], A[i * 3 + 2], B[j], B[3 + j], B[6 + j]) for i in range(3) for j in range(3)]


def _sqrt(x):
    return float(np.sqrt(np.float64(x)))  # NaN for a negative argument, as the C sqrt


def quat_from_R(R):
    q = [0.0] * 4
    t = (R[0] + R[4]) + R[8]
    if t > 0.0:
        t = _sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
    elif R[0] >= R[4] and R[0] >= R[8]:
        t = _sqrt(((R[0] - R[4]) - R[8]) + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[3], q[1], q[2] = (R[7] - R[5]) * t, (R[3] + R[1]) * t, (R[6] + R[2]) * t
    elif R[4] > R[0] and R[4] >= R[8]:
        t = _sqrt(((R[4] - R[8]) - R[0]) + 1.0)
        q[1] = 0.5 * t
        t = 0.5 / t
        q[3], q[2], q[0] = (R[2] - R[6]) * t, (R[7] + R[5]) * t, (R[1] + R[3]) * t
    else:
        t = _sqrt(((R[8] - R[0]) - R[4]) + 1.0)
        q[2] = 0.5 * t
        t = 0.5 / t
        q[3], q[0], q[1] = (R[3] - R[1]) * t, (R[2] + R[6]) * t, (R[5] + R[7]) * t
    return q


def _div(a, b):
    return float(np.float64(a) / np.float64(b))  # IEEE division: inf / NaN instead of ZeroDivisionError


def quat_normalize(q):
    if q[3] < 0.0:
        q = [-v for v in q]
    n = _sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [_div(v, n) for v in q]


def quat_to_R(q):
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


class Pose:
    def __init__(self, q, t):
        self.q, self.t, self.R = list(q), list(t), quat_to_R(q)


def pose_from_floats(Rcw, tcw):
    q = quat_normalize(quat_from_R([float(v) for v in Rcw]))
    return Pose(q, [float(v) for v in tcw])


def pose_update(T, x):
    with np.errstate(all="ignore"):
        ox, oy, oz = x[0], x[1], x[2]
        theta = _sqrt((ox * ox + oy * oy) + oz * oz)
        Om = [0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0]
        Om2 = mat3_mul(Om, Om)
        ident = [1.0 if i % 4 == 0 else 0.0 for i in range(9)]
        if theta < 0.00001:
            R = [(ident[i] + Om[i]) + Om2[i] for i in range(9)]
            V = R
        else:
            s, c = sin_cos(theta)
            th2 = theta * theta
            a, b, g = _div(s, theta), _div(1.0 - c, th2), _div(theta - s, th2 * theta)
            R = [(ident[i] + a * Om[i]) + b * Om2[i] for i in range(9)]
            V = [(ident[i] + b * Om[i]) + g * Om2[i] for i in range(9)]
        qe = quat_normalize(quat_from_R(R))
        Re = quat_to_R(qe)
        te = [dot3(V[i * 3], V[i * 3 + 1], V[i * 3 + 2], x[3], x[4], x[5]) for i in range(3)]
        t = [te[i] + dot3(Re[i * 3], Re[i * 3 + 1], Re[i * 3 + 2], T.t[0], T.t[1], T.t[2]) for i in range(3)]
        a, b = qe, T.q
        q = [((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1],
             ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2],
             ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0],
             ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]]
        return Pose(quat_normalize(q), t)


class Cam:
    def __init__(self, camera):
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(camera[k]) for k in ("fx", "fy", "cx", "cy", "mbf"))


class Edges:
    """the compact edge list of one frame: float32 fields widened to float64 arrays, in ascending feature order"""
    def __init__(self, feat, u, v, ur, pos, w):
        self.feat = np.asarray(feat, np.int64)
        self.u, self.v, self.ur, self.w = (np.asarray(a, np.float32).astype(np.float64) for a in (u, v, ur, w))
        pos = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64)
        self.X, self.Y, self.Z = pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy()
        self.stereo = ~(self.ur < 0.0)
        self.n = len(self.feat)


def edge_error(T, cam, E):
    """-> pc (3 arrays), e (3 arrays), chi2"""
    R, t = T.R, T.t
    pc = [((R[i * 3] * E.X + R[i * 3 + 1] * E.Y) + R[i * 3 + 2] * E.Z) + t[i] for i in range(3)]
    m0 = E.u - ((pc[0] / pc[2]) * cam.fx + cam.cx)
    m1 = E.v - ((pc[1] / pc[2]) * cam.fy + cam.cy)
    invz = (1.0 / pc[2]).astype(np.float32).astype(np.float64)
    r0 = (pc[0] * invz) * cam.fx + cam.cx
    s0 = E.u - r0
    s1 = E.v - ((pc[1] * invz) * cam.fy + cam.cy)
    s2 = E.ur - (r0 - cam.bf * invz)
    st = E.stereo
    e = [np.where(st, s0, m0), np.where(st, s1, m1), np.where(st, s2, 0.0)]
    c2 = e[0] * (E.w * e[0]) + e[1] * (E.w * e[1])
    chi2 = np.where(st, c2 + e[2] * (E.w * e[2]), c2)
    return pc, e, chi2


def robustify(chi2, stereo, huber):
    delta = np.where(stereo, DELTA_STEREO, DELTA_MONO)
    dsqr = delta * delta
    plain = (chi2 <= dsqr) if huber else np.ones(len(chi2), bool)
    sqrte = np.sqrt(chi2)
    rho0 = np.where(plain, chi2, (2.0 * sqrte) * delta - dsqr)
    rho1 = np.where(plain, 1.0, delta / sqrte)
    return rho0, rho1


def strided_partials(terms, active, subtract=False):
    acc = np.zeros(K_THREADS)
    for j in range(0, len(terms), K_THREADS):
        seg, m = terms[j:j + K_THREADS], active[j:j + K_THREADS]
        cur = acc[:len(seg)]
        acc[:len(seg)] = np.where(m, cur - seg if subtract else cur + seg, cur)
    return acc


def tree_sum(p):
    p = np.array(p, np.float64).reshape(K_THREADS // 64, 64)
    s = 32
    while s > 0:
        p[:, :s] = p[:, :s] + p[:, s:2 * s]
        s >>= 1
    B = [float(v) for v in p[:, 0]]
    return (B[0] + B[1]) + (B[2] + B[3])


def linearise(T, cam, E, active, huber):
    """-> the 28 sums of edge_accumulate over the active edges"""
    pc, e, chi2 = edge_error(T, cam, E)
    rho0, rho1 = robustify(chi2, E.stereo, huber)
    x, y = pc[0], pc[1]
    invz = 1.0 / pc[2]
    invz2 = invz * invz
    fx, fy, bf, w, st = cam.fx, cam.fy, cam.bf, E.w, E.stereo
    zero = np.zeros(E.n)
    J = [[None] * 6 for _ in range(3)]
    J[0][0] = ((x * y) * invz2) * fx
    J[0][1] = (-(1.0 + (x * x) * invz2)) * fx
    J[0][2] = (y * invz) * fx
    J[0][3] = (-invz) * fx
    J[0][4] = zero
    J[0][5] = (x * invz2) * fx
    J[1][0] = (1.0 + (y * y) * invz2) * fy
    J[1][1] = (((-x) * y) * invz2) * fy
    J[1][2] = ((-x) * invz) * fy
    J[1][3] = zero
    J[1][4] = (-invz) * fy
    J[1][5] = (y * invz2) * fy
    J[2][0] = J[0][0] - (bf * y) * invz2
    J[2][1] = J[0][1] + (bf * x) * invz2
    J[2][2] = J[0][2]
    J[2][3] = J[0][3]
    J[2][4] = zero
    J[2][5] = J[0][5] - bf * invz2
    wr = rho1 * w
    we = [w * e[0], w * e[1], w * e[2]]
    sums = []
    for a in range(6):
        for b in range(a, 6):
            h = (J[0][a] * wr) * J[0][b] + (J[1][a] * wr) * J[1][b]
            h = np.where(st, h + (J[2][a] * wr) * J[2][b], h)
            sums.append(tree_sum(strided_partials(h, active)))
    for a in range(6):
        g = J[0][a] * we[0] + J[1][a] * we[1]
        g = np.where(st, g + J[2][a] * we[2], g)
        sums.append(tree_sum(strided_partials(rho1 * g, active, subtract=True)))
    sums.append(tree_sum(strided_partials(rho0, active)))
    return sums


def robust_chi2_sum(T, cam, E, active, huber):
    _, _, chi2 = edge_error(T, cam, E)
    rho0, _ = robustify(chi2, E.stereo, huber)
    return tree_sum(strided_partials(rho0, active))


def solve6(H, lam, b, x):
    """-> (ok, x): x is the argument itself when a pivot is negative"""
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = H[k] + lam if i == j else H[k]
            k += 1
    perm = list(range(6))
    ok = True
    for k in range(6):
        best, bv = k, abs(A[k][k])
        for i in range(k + 1, 6):
            v = abs(A[i][i])
            if v > bv:
                bv, best = v, i
        if best != k:
            A[k], A[best] = A[best], A[k]
            for j in range(6):
                A[j][k], A[j][best] = A[j][best], A[j][k]
            perm[k], perm[best] = perm[best], perm[k]
        d = A[k][k]
        if d < 0.0:
            ok = False
        if abs(d) > TINY:
            for i in range(k + 1, 6):
                A[i][k] = _div(A[k][i], d)
            for j in range(k + 1, 6):
                for i in range(j, 6):
                    A[j][i] = A[i][j] = A[i][j] - A[i][k] * A[k][j]
        else:
            for i in range(k + 1, 6):
                A[i][k] = 0.0
    if not ok:
        return False, x
    y = [b[perm[i]] for i in range(6)]
    for i in range(1, 6):
        for j in range(i):
            y[i] = y[i] - A[i][j] * y[j]
    for i in range(6):
        y[i] = _div(y[i], A[i][i]) if abs(A[i][i]) > TINY else 0.0
    for i in range(4, -1, -1):
        for j in range(i + 1, 6):
            y[i] = y[i] - A[j][i] * y[j]
    out = [0.0] * 6
    for i in range(6):
        out[perm[i]] = y[i]
    return True, out


class Lm:
    def __init__(self, init):
        self.cur = self.trial = self.last_eval = init
        self.x = [0.0] * 6
        self.lam, self.ni, self.current_chi, self.ini_chi, self.rho = 0.0, 2.0, 0.0, 0.0, 0.0
        self.n_bad = self.qmax = self.iter = self.trials = 0
        self.solved = False

    def make_trial(self):
        self.solved, self.x = solve6(self.H, self.lam, self.b, self.x)
        self.trial = pose_update(self.cur, self.x)

    def iteration_begin(self, sums):
        self.H, self.b = sums[:21], sums[21:27]
        self.current_chi = self.ini_chi = sums[27]
        self.last_eval = self.cur
        if self.iter == 0:
            m, k = 0.0, 0
            for j in range(6):
                a = abs(self.H[k])
                m = m if a < m else a
                k += 6 - j
            self.lam, self.ni, self.n_bad = 1e-5 * m, 2.0, 0
        self.rho, self.qmax = 0.0, 0
        self.make_trial()

    def trial_done(self, chi_sum):
        with np.errstate(all="ignore"):
            temp = chi_sum if self.solved else DBL_MAX
            self.last_eval = self.trial
            scale = 0.0
            for j in range(6):
                scale = scale + self.x[j] * (self.lam * self.x[j] + self.b[j])
            scale = scale + 1e-3
            self.rho = _div(float(np.float64(self.current_chi) - np.float64(temp)), scale)
            if self.rho > 0.0 and float(np.float64(temp) - np.float64(temp)) == 0.0:
                t = 2.0 * self.rho - 1.0
                alpha = 1.0 - float((np.float64(t) * np.float64(t)) * np.float64(t))
                alpha = (2.0 / 3.0) if (2.0 / 3.0) < alpha else alpha
                f = alpha if (1.0 / 3.0) < alpha else (1.0 / 3.0)
                self.lam = self.lam * f
                self.ni = 2.0
                self.current_chi = temp
                self.cur = self.trial
            else:
                self.lam = float(np.float64(self.lam) * np.float64(self.ni))
                self.ni = self.ni * 2.0
            self.qmax += 1
            self.trials += 1
            if self.rho < 0.0 and self.qmax < K_TRIALS:
                self.make_trial()
                return ACT_TRIAL
            self.iter += 1
            if self.qmax == K_TRIALS or self.rho == 0.0:
                return ACT_ROUND_END
            if float(np.float64(self.ini_chi - self.current_chi) * np.float64(1e3)) < self.ini_chi:
                self.n_bad += 1
            else:
                self.n_bad = 0
            if self.n_bad >= 3 or self.iter == K_ITERATIONS:
                return ACT_ROUND_END
            return ACT_ITERATE


def pose_store(Rt):
    """-> Tcw [12] float32 (rows of R | t), Ow [3] float32"""
    Tcw = np.zeros(12, np.float32)
    for i in range(3):
        for j in range(3):
            Tcw[i * 4 + j] = np.float32(Rt[i * 3 + j])
        Tcw[i * 4 + 3] = np.float32(Rt[9 + i])
    d = [float(v) for v in Tcw]
    Ow = np.array([np.float32(-dot3(d[i], d[4 + i], d[8 + i], d[3], d[7], d[11])) for i in range(3)], np.float32)
    return Tcw, Ow


def optimize_edges(E, camera, status=0, trace=None):
    """amos_pose_core.h's optimize_host -> (RESULT record, outlier flag per edge or None when fewer than 3 edges)"""
    with np.errstate(all="ignore"):
        res = np.zeros(1, RESULT)[0]
        Rcw, tcw = camera["Rcw"], camera["tcw"]
        Rt = [float(v) for v in Rcw] + [float(v) for v in tcw]
        res["n_edges"], res["status"] = E.n, status
        if E.n < 3:
            res["Rt"] = Rt
            res["Tcw"], res["Ow"] = pose_store(Rt)
            return res, None
        cam = Cam(camera)
        init = pose_from_floats(Rcw, tcw)
        outlier = np.zeros(E.n, bool)
        n_bad = 0
        for rnd in range(K_ROUNDS):
            huber = rnd < 3
            s = Lm(init)
            active = ~outlier
            act = ACT_ITERATE if active.any() else ACT_ROUND_END
            while act != ACT_ROUND_END:
                s.iteration_begin(linearise(s.cur, cam, E, active, huber))
                while True:
                    act = s.trial_done(robust_chi2_sum(s.trial, cam, E, active, huber))
                    if act != ACT_TRIAL:
                        break
            _, _, chi_cur = edge_error(s.cur, cam, E)
            _, _, chi_last = edge_error(s.last_eval, cam, E)
            chi2 = np.where(outlier, chi_cur, chi_last)
            if trace is not None:
                trace.append(dict(chi2=chi2.copy(), pose=s.cur))
            outlier = chi2.astype(np.float32) > np.where(E.stereo, CHI2_STEREO, CHI2_MONO)
            n_bad = int(outlier.sum())
            res["rounds"] = rnd + 1
            res["iterations"][rnd], res["trials"][rnd], res["lambda"][rnd], res["chi2"][rnd] = s.iter, s.trials, s.lam, s.current_chi
            Rt = list(s.cur.R) + list(s.cur.t)
            if E.n < 10:
                break
        res["Rt"] = Rt
        res["Tcw"], res["Ow"] = pose_store(Rt)
        res["n_inliers"] = E.n - n_bad
        return res, outlier


def gather_edges(kps, u_right, match, pos, inv_sigma2, count=None):
    """The kernel's prologue: features i < count with match[i] >= 0 in ascending order -> (Edges, status).  pos: [points][3]."""
    n = len(kps) if count is None else min(int(count), len(kps))
    match = np.asarray(match, np.int32)[:n]
    octv = kps["octave"][:n]
    has = match >= 0
    bad_oct = has & ((octv < 0) | (octv >= len(inv_sigma2)))
    bad_idx = has & (match >= len(pos))
    status = (STATUS_OCTAVE if bad_oct.any() else 0) | (STATUS_MATCH_INDEX if bad_idx.any() else 0)
    feat = np.nonzero(has & ~bad_oct & ~bad_idx)[0]
    ur = np.full(len(feat), -1.0, np.float32) if u_right is None else np.asarray(u_right, np.float32)[feat]
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    w = np.asarray(inv_sigma2, np.float32)[octv[feat]]
    return Edges(feat, kps["x"][feat], kps["y"][feat], ur, pos[match[feat]], w), status


def pose_optimization(kps, u_right, match, pos, has_obs, camera, inv_sigma2, outlier_in, clear_outliers, count=None):
    """One frame as amos_match_pose_optimization_batch_device leaves it -> (RESULT record, outlier bytes, match).  has_obs: one bool per
    point or None (every point counts); outlier_in: the bytes d_outlier held on entry (features without an edge keep them)."""
    E, status = gather_edges(kps, u_right, match, pos, inv_sigma2, count)
    res, flags = optimize_edges(E, camera, status)
    outlier = np.array(outlier_in, np.uint8)
    match = np.array(match, np.int32)
    if flags is None:
        return res, outlier, match
    outlier[E.feat] = flags
    keep = E.feat[~flags]
    res["n_inliers_with_obs"] = len(keep) if has_obs is None else int(np.asarray(has_obs, bool)[match[keep]].sum())
    if clear_outliers:
        match[E.feat[flags]] = -1
        outlier[E.feat[flags]] = 0
    return res, outlier, match
