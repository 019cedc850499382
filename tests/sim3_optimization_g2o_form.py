"""Optimizer::OptimizeSim3 written straight from the g2o text, independent of amos_sim3_opt_core.h's restatement: the sums run edge after edge,
Sim3::map rotates by the quaternion and scales afterwards, inverse() is taken where an edge needs it, sines, cosines and the exponential are
math's, the linear system goes to numpy.linalg.  It shares only the gathering (sim3_optimization_restatement.gather) with the restatement.
The per-edge arithmetic is vectorised over the edges (one edge per array element); the sums over them are plain loops."""
import math

import numpy as np


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def qrot(q, v):
    """Eigen's QuaternionBase::_transformVector; v: [..., 3]"""
    uv = 2.0 * np.cross(q[:3], v)
    return v + q[3] * uv + np.cross(q[:3], uv)


def quat_of(R):
    """Eigen::Quaterniond(Matrix3d), not normalised"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3], q[j], q[k] = (R[k, j] - R[j, k]) * t, (R[j, i] + R[i, j]) * t, (R[k, i] + R[i, k]) * t
    return q


class Sim3:
    def __init__(self, q, t, s):
        self.q, self.t, self.s = np.asarray(q, float), np.asarray(t, float), float(s)

    @staticmethod
    def exp(update):
        omega, upsilon, sigma = update[:3], update[3:6], update[6]
        theta = math.sqrt(float(omega @ omega))
        Om = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]])
        s = math.exp(sigma)
        Om2, I, eps = Om @ Om, np.eye(3), 0.00001
        if abs(sigma) < eps:
            C = 1.0
            if theta < eps:
                A, B, R = 1.0 / 2.0, 1.0 / 6.0, I + Om + Om @ Om
            else:
                theta2 = theta * theta
                A, B = (1 - math.cos(theta)) / theta2, (theta - math.sin(theta)) / (theta2 * theta)
                R = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
        else:
            C = (s - 1) / sigma
            if theta < eps:
                sigma2 = sigma * sigma
                A, B, R = ((sigma - 1) * s + 1) / sigma2, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), I + Om + Om2
            else:
                R = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
                a, b, theta2, sigma2 = s * math.sin(theta), s * math.cos(theta), theta * theta, sigma * sigma
                c = theta2 + sigma2
                A, B = (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
        W = A * Om + B * Om2 + C * I
        return Sim3(quat_of(R), W @ upsilon, s)

    def map(self, xyz):
        return self.s * qrot(self.q, xyz) + self.t

    def inverse(self):
        qc = np.array([-self.q[0], -self.q[1], -self.q[2], self.q[3]])
        return Sim3(qc, qrot(qc, (-1.0 / self.s) * self.t), 1.0 / self.s)

    def __mul__(self, o):
        return Sim3(qmul(self.q, o.q), self.s * qrot(self.q, o.t) + self.t, self.s * o.s)


def oplus(est, update, fix_scale):
    update = np.array(update, float)
    if fix_scale:
        update[6] = 0
    return Sim3.exp(update) * est


def errors(est, cams, C):
    """computeError of both edges of every correspondence -> e12 [n][2], e21 [n][2]"""
    P1, P2 = np.stack(C.P1, 1), np.stack(C.P2, 1)
    o1, o2 = np.stack(C.o1, 1), np.stack(C.o2, 1)
    out = []
    for S, K, X, obs in ((est, cams[0], P2, o1), (est.inverse(), cams[1], P1, o2)):
        p = S.map(X)
        proj = p[:, :2] / p[:, 2:3]
        out.append(obs - (proj * np.array(K[:2]) + np.array(K[2:])))
    return out


def jacobians(est, cams, C, fix_scale):
    """BaseBinaryEdge::linearizeOplus, the numeric central difference -> J12, J21 [n][2][7]"""
    delta = 1e-9
    scalar = 1.0 / (2 * delta)
    J = [np.zeros((C.n, 2, 7)), np.zeros((C.n, 2, 7))]
    for d in range(7):
        add = np.zeros(7)
        add[d] = delta
        ep = errors(oplus(est, add, fix_scale), cams, C)
        add[d] = -delta
        em = errors(oplus(est, add, fix_scale), cams, C)
        for k in range(2):
            J[k][:, :, d] = scalar * (ep[k] - em[k])
    return J


def huber(e2, delta):
    dsqr = delta * delta
    if e2 <= dsqr:
        return e2, 1.0
    sqrte = math.sqrt(e2)
    return 2 * sqrte * delta - dsqr, delta / sqrte


def build(est, cams, C, active, delta, fix_scale):
    e = errors(est, cams, C)
    J = jacobians(est, cams, C, fix_scale)
    H, b, chi = np.zeros((7, 7)), np.zeros(7), 0.0
    for c in range(C.n):
        if not active[c]:
            continue
        for k, w in ((0, C.w1[c]), (1, C.w2[c])):
            err = e[k][c]
            rho0, rho1 = huber(float(err @ (w * err)), delta)
            B = J[k][c]
            b += B.T @ (rho1 * (-(w * err)))
            H += B.T @ ((rho1 * w) * B)
            chi += rho0
    return H, b, chi


def robust_chi2(est, cams, C, active, delta):
    e = errors(est, cams, C)
    chi = 0.0
    for c in range(C.n):
        if active[c]:
            chi += huber(float(e[0][c] @ (C.w1[c] * e[0][c])), delta)[0] + huber(float(e[1][c] @ (C.w2[c] * e[1][c])), delta)[0]
    return chi


def levenberg(est, cams, C, active, delta, fix_scale, max_iter):
    """SparseOptimizer::optimize(max_iter) with OptimizationAlgorithmLevenberg -> (estimate, the estimate the errors were last computed at)"""
    lam, ni, n_bad, last = 0.0, 2.0, 0, est
    for it in range(max_iter):
        H, b, chi = build(est, cams, C, active, delta, fix_scale)
        last = est
        ini = chi
        if it == 0:
            lam, ni = 1e-5 * np.abs(np.diag(H)).max(), 2.0
        rho, qmax = 0.0, 0
        while True:
            A = H + lam * np.eye(7)
            ok = bool(np.all(np.linalg.eigvalsh(A) >= 0))
            trial = est
            if ok:
                x = np.linalg.solve(A, b)
                trial = oplus(est, x, fix_scale)
                temp = robust_chi2(trial, cams, C, active, delta)
                last = trial
            else:
                x, temp = np.zeros(7), 1.7976931348623157e308
            rho = (chi - temp) / (float(x @ (lam * x + b)) + 1e-3)
            if rho > 0 and math.isfinite(temp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni, chi, est = 2.0, temp, trial
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            break
        n_bad = n_bad + 1 if (ini - chi) * 1e3 < ini else 0
        if n_bad >= 3:
            break
    return est, last


def optimize(C, pair, cam1, cam2):
    """-> dict(n_inliers, n_bad_first, bad [n], q, t, s) -- Optimizer.cc:1364-1590 on the gathered correspondences"""
    fix, th2 = int(pair["fix_scale"]), float(np.float32(pair["th2"]))
    est = Sim3(quat_of(np.asarray(pair["R12"], np.float32).astype(float).reshape(3, 3)), pair["t12"].astype(float), float(pair["s12"]))
    cams = [[float(c[k]) for k in ("fx", "fy", "cx", "cy")] for c in (cam1, cam2)]
    delta = float(np.float32(math.sqrt(th2)))
    bad = np.zeros(C.n, bool)
    out = dict(n_inliers=0, n_bad_first=0, bad=bad, q=est.q, t=est.t, s=est.s)
    if C.n == 0:
        return out

    def classify(at, active):
        e12, e21 = errors(at, cams, C)
        c12, c21 = C.w1 * (e12 * e12).sum(1), C.w2 * (e21 * e21).sum(1)
        return active & ((c12 > th2) | (c21 > th2))

    cur, last = levenberg(est, cams, C, ~bad, delta, fix, 5)
    first = classify(last, ~bad)
    bad |= first
    out["n_bad_first"] = int(first.sum())
    if C.n - out["n_bad_first"] < 10:
        return out
    cur, last = levenberg(cur, cams, C, ~bad, delta, fix, 10 if out["n_bad_first"] > 0 else 5)
    second = classify(last, ~bad)
    out["n_inliers"] = int((~bad).sum() - second.sum())
    bad |= second
    out["q"], out["t"], out["s"] = cur.q, cur.t, cur.s
    return out
