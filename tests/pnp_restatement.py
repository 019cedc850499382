"""tests/pnp_restatement.py -- cv::solvePnPRansac(obj, img, K, 0, ..., SOLVEPNP_P3P) as amos-slam_amd/csrc/amos_pnp_core.h restates it
(OpenCV 4.5's RANSACPointSetRegistrator with 4-point samples + PnPRansacCallback, p3p.cpp, then the EPnP refit of epnp.cpp on the RANSAC
inliers; written from memory of the published source: parity with OpenCV unpinned), in Python floats -- IEEE doubles without fused
multiply-add, the same operations in the same order.  TEST INFRASTRUCTURE ONLY: the GPU tests hold amos_pnp_ransac_device to it bit for
bit.  The scoring of every model over every point is numpy (elementwise, one rounding per operation, the order of the kernel); every sum
over points runs from 0.0 in index order."""
import math

import numpy as np

from fmat_restatement import REDRAW_CAP, BISECT, Rng, _abs, _div, _sqrt, log_, round_even, DBL_MIN

MODEL_POINTS = 4
JACOBI_SWEEPS = 50
PINV_CUT = 1e-14
f32 = np.float32


def _finite(x):
    return x - x == 0


def update_num_iters(p, ep, max_iters):
    """RANSACUpdateNumIters(p, ep, 4, max_iters)."""
    p = 0.0 if p < 0 else (1.0 if p > 1 else p)
    ep = 0.0 if ep < 0 else (1.0 if ep > 1 else ep)
    num = 1.0 - p
    if num < DBL_MIN:
        num = DBL_MIN
    q = 1.0 - ep
    q2 = q * q
    denom = 1.0 - q2 * q2
    if denom < DBL_MIN:
        return 0
    num, denom = log_(num), log_(denom)
    return max_iters if (denom >= 0 or -num >= float(max_iters) * -denom) else round_even(_div(num, denom))


def errors(Rt, obj, img, fx, fy, cx, cy):
    """PnPRansacCallback::computeError (k_pnp_score's arithmetic) for every point: float32 [n]."""
    M = [float(v) for v in np.asarray(Rt, np.float64).reshape(12)]
    X, Y, Z = (obj[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        xc = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[9]
        yc = ((M[3] * X + M[4] * Y) + M[5] * Z) + M[10]
        zc = ((M[6] * X + M[7] * Y) + M[8] * Z) + M[11]
        zc = np.where(zc != 0.0, 1.0 / np.where(zc != 0.0, zc, 1.0), 1.0)
        xn, yn = xc * zc, yc * zc
        u = (xn * fx + cx).astype(np.float32)
        v = (yn * fy + cy).astype(np.float32)
        dx, dy = img[:, 0] - u, img[:, 1] - v
        return dx * dx + dy * dy


# ---- image points (undistort_normalised with zero distortion: x = (u - cx) * (1 / fx), exactly)
def normalised(u, fx, cx):
    return (float(u) - cx) * _div(1.0, fx)


def pixel_p3p(u, fx, cx):
    return float(f32(normalised(u, fx, cx))) * fx + cx


def pixel_refit(u, fx, cx):
    return normalised(u, fx, cx) * fx + cx


# ---- polynomial roots
def poly_at(c, x):
    acc = x + c[0]
    for k in range(1, len(c)):
        acc = acc * x + c[k]
    return acc


def poly_bisect(c, lo, hi, increasing):
    for _ in range(BISECT):
        mid = lo * 0.5 + hi * 0.5
        if not (lo < mid < hi):
            break
        if (poly_at(c, mid) > 0) == increasing:
            hi = mid
        else:
            lo = mid
    return lo * 0.5 + hi * 0.5


def roots_between(c, pts):
    out = []
    flo = poly_at(c, pts[0])
    for k in range(len(pts) - 1):
        lo, hi = pts[k], pts[k + 1]
        fhi = poly_at(c, hi)
        if flo == 0:
            if not out or out[-1] != lo:
                out.append(lo)
        elif (flo < 0 and fhi > 0) or (flo > 0 and fhi < 0):
            out.append(poly_bisect(c, lo, hi, flo < 0))
        flo = fhi
    return out


def _clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def solve_quartic(a, b, c, d, e):
    """Real roots of a x^4 + b x^3 + c x^2 + d x + e (a != 0), ascending."""
    q = [_div(b, a), _div(c, a), _div(d, a), _div(e, a)]
    if not all(_finite(v) for v in q):
        return []
    B4 = _abs(q[0])
    for v in q[1:]:
        B4 = _abs(v) if _abs(v) > B4 else B4
    B4 = B4 + 1.0
    c3 = [0.75 * q[0], 0.5 * q[1], 0.25 * q[2]]
    B3 = _abs(c3[0])
    for v in c3[1:]:
        B3 = _abs(v) if _abs(v) > B3 else B3
    B3 = B3 + 1.0
    p3 = [-B3]
    disc = c3[0] * c3[0] - 3.0 * c3[1]
    if disc > 0:
        s = _sqrt(disc)
        m1 = _clamp(_div(-c3[0] - s, 3.0), -B3, B3)
        m2 = _clamp(_div(-c3[0] + s, 3.0), m1, B3)
        p3 += [m1, m2]
    p3.append(B3)
    crit = roots_between(c3, p3)
    p4 = [-B4]
    for r in crit:
        p4.append(_clamp(r, p4[-1], B4))
    p4.append(B4)
    return roots_between(q, p4)


# ---- symmetric eigen-decomposition
def jacobi_sym(A):
    """A: [n][n] float64 (copied) -> (diagonal after the sweeps, V with eigenvectors as columns, signs fixed)."""
    A = np.array(A, np.float64)
    n = len(A)
    V = np.eye(n)
    for _ in range(JACOBI_SWEEPS):
        off = 0.0
        for p in range(n):
            for q in range(p + 1, n):
                off = off + _abs(float(A[p, q]))
        if not off > 0:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = float(A[p, q])
                if apq == 0:
                    continue
                app, aqq = float(A[p, p]), float(A[q, q])
                g = 100.0 * _abs(apq)
                if _abs(app) + g == _abs(app) and _abs(aqq) + g == _abs(aqq):
                    A[p, q] = A[q, p] = 0.0
                    continue
                theta = _div(aqq - app, 2.0 * apq)
                t = _div(1.0, _abs(theta) + _sqrt(theta * theta + 1.0))
                if theta < 0:
                    t = -t
                c = _div(1.0, _sqrt(t * t + 1.0))
                s = t * c
                kp, kq = A[:, p].copy(), A[:, q].copy()
                A[:, p] = c * kp - s * kq
                A[:, q] = s * kp + c * kq
                pk, qk = A[p, :].copy(), A[q, :].copy()
                A[p, :] = c * pk - s * qk
                A[q, :] = s * pk + c * qk
                A[p, q] = A[q, p] = 0.0
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = c * vp - s * vq
                V[:, q] = s * vp + c * vq
    for k in range(n):
        im = 0
        for i in range(1, n):
            im = i if _abs(V[i, k]) > _abs(V[im, k]) else im
        if V[im, k] < 0:
            V[:, k] = -V[:, k]
    return [float(A[i, i]) for i in range(n)], V


def eig_order(lam, desc):
    used, order = set(), []
    for _ in range(len(lam)):
        best = -1
        for i in range(len(lam)):
            if i in used:
                continue
            if best < 0 or (lam[i] > lam[best] if desc else lam[i] < lam[best]):
                best = i
        used.add(best)
        order.append(best)
    return order


# ---- P3P
def jacobi_4x4(A):
    A = list(A)
    U = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    B = [A[0], A[5], A[10], A[15]]
    D = list(B)
    Z = [0.0] * 4
    for it in range(50):
        sm = ((((_abs(A[1]) + _abs(A[2])) + _abs(A[3])) + _abs(A[6])) + _abs(A[7])) + _abs(A[11])
        if sm == 0.0:
            return D, U
        tresh = _div(0.2 * sm, 16.0) if it < 3 else 0.0
        for i in range(3):
            for j in range(i + 1, 4):
                Aij = A[4 * i + j]
                eps_machine = 100.0 * _abs(Aij)
                if it > 3 and _abs(D[i]) + eps_machine == _abs(D[i]) and _abs(D[j]) + eps_machine == _abs(D[j]):
                    A[4 * i + j] = 0.0
                elif _abs(Aij) > tresh:
                    hh = D[j] - D[i]
                    if _abs(hh) + eps_machine == _abs(hh):
                        t = _div(Aij, hh)
                    else:
                        theta = _div(0.5 * hh, Aij)
                        t = _div(1.0, _abs(theta) + _sqrt(1.0 + theta * theta))
                        if theta < 0.0:
                            t = -t
                    hh = t * Aij
                    Z[i] -= hh
                    Z[j] += hh
                    D[i] -= hh
                    D[j] += hh
                    A[4 * i + j] = 0.0
                    c = _div(1.0, _sqrt(1 + t * t))
                    s = t * c
                    tau = _div(s, 1.0 + c)
                    for k in range(0, i):
                        g, h = A[k * 4 + i], A[k * 4 + j]
                        A[k * 4 + i] = g - s * (h + g * tau)
                        A[k * 4 + j] = h + s * (g - h * tau)
                    for k in range(i + 1, j):
                        g, h = A[i * 4 + k], A[k * 4 + j]
                        A[i * 4 + k] = g - s * (h + g * tau)
                        A[k * 4 + j] = h + s * (g - h * tau)
                    for k in range(j + 1, 4):
                        g, h = A[i * 4 + k], A[j * 4 + k]
                        A[i * 4 + k] = g - s * (h + g * tau)
                        A[j * 4 + k] = h + s * (g - h * tau)
                    for k in range(4):
                        g, h = U[k * 4 + i], U[k * 4 + j]
                        U[k * 4 + i] = g - s * (h + g * tau)
                        U[k * 4 + j] = h + s * (g - h * tau)
        for i in range(4):
            B[i] += Z[i]
            D[i] = B[i]
            Z[i] = 0.0
    return D, U


def align(M, P):
    Ce = [_div((M[0][i] + M[1][i]) + M[2][i], 3) for i in range(3)]
    Cs = [_div((P[0][i] + P[1][i]) + P[2][i], 3) for i in range(3)]
    s = [0.0] * 9
    for j in range(3):
        for i in range(3):
            s[i * 3 + j] = _div((P[0][i] * M[0][j] + P[1][i] * M[1][j]) + P[2][i] * M[2][j], 3) - Ce[j] * Cs[i]
    Q = [0.0] * 16
    Q[0] = (s[0] + s[4]) + s[8]
    Q[5] = (s[0] - s[4]) - s[8]
    Q[10] = (s[4] - s[8]) - s[0]
    Q[15] = (s[8] - s[0]) - s[4]
    Q[4] = Q[1] = s[5] - s[7]
    Q[8] = Q[2] = s[6] - s[2]
    Q[12] = Q[3] = s[1] - s[3]
    Q[9] = Q[6] = s[3] + s[1]
    Q[13] = Q[7] = s[6] + s[2]
    Q[14] = Q[11] = s[7] + s[5]
    evs, U = jacobi_4x4(Q)
    iev, evmax = 0, evs[0]
    for i in range(1, 4):
        if evs[i] > evmax:
            iev = i
            evmax = evs[i]
    q = [U[i * 4 + iev] for i in range(4)]
    q02, q12, q22, q32 = q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]
    q0_1, q0_2, q0_3 = q[0] * q[1], q[0] * q[2], q[0] * q[3]
    q1_2, q1_3, q2_3 = q[1] * q[2], q[1] * q[3], q[2] * q[3]
    R = [((q02 + q12) - q22) - q32, 2. * (q1_2 - q0_3), 2. * (q1_3 + q0_2),
         2. * (q1_2 + q0_3), ((q02 + q22) - q12) - q32, 2. * (q2_3 - q0_1),
         2. * (q1_3 - q0_2), 2. * (q2_3 + q0_1), ((q02 + q32) - q12) - q22]
    t = [Ce[i] - ((R[3 * i] * Cs[0] + R[3 * i + 1] * Cs[1]) + R[3 * i + 2] * Cs[2]) for i in range(3)]
    return R + t


def solve_for_lengths(distances, cosines):
    p, q, r = cosines[0] * 2, cosines[1] * 2, cosines[2] * 2
    inv_d22 = _div(1., distances[2] * distances[2])
    a = inv_d22 * (distances[0] * distances[0])
    b = inv_d22 * (distances[1] * distances[1])
    a2, b2, p2, q2, r2 = a * a, b * b, p * p, q * q, r * r
    pr = p * r
    pqr = q * pr
    if p2 + q2 + r2 - pqr - 1 == 0:
        return []
    ab, a_2 = a * b, 2 * a
    A = -2 * b + b2 + a2 + 1 + ab * (2 - r2) - a_2
    if A == 0:
        return []
    a_4 = 4 * a
    B = q * (-2 * (ab + a2 + 1 - b) + r2 * ab + a_4) + pr * (b - b2 + ab)
    C = q2 + b2 * (r2 + p2 - 2) - b * (p2 + pqr) - ab * (r2 + pqr) + (a2 - a_2) * (2 + q2) + 2
    D = pr * (ab - b2 + b) + q * ((p2 - 2) * b + 2 * (ab - a2) + a_4 - 2)
    E = 1 + 2 * (b - a - ab) + b2 - b * p2 + a2
    temp = p2 * (a - 1 + b) + r2 * (a - 1 - b) + pqr - a * pqr
    b0 = b * temp * temp
    if b0 == 0:
        return []
    roots = solve_quartic(A, B, C, D, E)
    if not roots:
        return []
    r3 = r2 * r
    pr2 = p * r2
    r3q = r3 * q
    inv_b0 = _div(1., b0)
    out = []
    for x in roots:
        if x <= 0:
            continue
        x2 = x * x
        b1 = (((1 - a - b) * x2 + (q * a - q) * x + 1 - a + b) *
              (((r3 * (a2 + ab * (2 - r2) - a_2 + b2 - 2 * b + 1)) * x +
                (r3q * (2 * (b - a2) + a_4 + ab * (r2 - 2) - 2) + pr2 * (1 + a2 + 2 * (ab - a - b) + r2 * (b - b2) + b2))) * x2 +
               (r3 * (q2 * (1 - 2 * a + a2) + r2 * (b2 - ab) - a_4 + 2 * (a2 - b2) + 2) + r * p2 * (b2 + 2 * (ab - b - a) + 1 + a2) +
                pr2 * q * (a_4 + 2 * (b - ab - a2) - 2 - r2 * b)) * x +
               2 * r3q * (a_2 - b - a2 + ab - 1) + pr2 * (q2 - a_4 + 2 * (a2 - b2) + r2 * b + q2 * (a2 - a_2) + 2) +
               p2 * (p * (2 * (ab - a - b) + a2 + b2 + 1) + 2 * q * r * (b + a_2 - a2 - ab - 1))))
        if b1 <= 0:
            continue
        y = inv_b0 * b1
        v = x2 + y * y - x * y * r
        if v <= 0:
            continue
        Zl = _div(distances[2], _sqrt(v))
        out.append((x * Zl, y * Zl, Zl))
    return out


def p3p_all(obj, img, fx, fy, cx, cy):
    """Every solution of the first three correspondences (list of 12-lists), as p3p4 computes them before its choice."""
    mu = [pixel_p3p(img[i][0], fx, cx) for i in range(4)]
    mv = [pixel_p3p(img[i][1], fy, cy) for i in range(4)]
    inv_fx, inv_fy, cx_fx, cy_fy = _div(1., fx), _div(1., fy), _div(cx, fx), _div(cy, fy)
    P = [[float(obj[i][j]) for j in range(3)] for i in range(3)]
    u, v, k = [0.0] * 3, [0.0] * 3, [0.0] * 3
    for i in range(3):
        u[i] = inv_fx * mu[i] - cx_fx
        v[i] = inv_fy * mv[i] - cy_fy
        norm = _sqrt(u[i] * u[i] + v[i] * v[i] + 1)
        k[i] = _div(1., norm)
        u[i] *= k[i]
        v[i] *= k[i]

    def d2(i, j):
        return ((P[i][0] - P[j][0]) * (P[i][0] - P[j][0]) + (P[i][1] - P[j][1]) * (P[i][1] - P[j][1])) + (P[i][2] - P[j][2]) * (P[i][2] - P[j][2])
    distances = [_sqrt(d2(1, 2)), _sqrt(d2(0, 2)), _sqrt(d2(0, 1))]
    cosines = [u[1] * u[2] + v[1] * v[2] + k[1] * k[2], u[0] * u[2] + v[0] * v[2] + k[0] * k[2], u[0] * u[1] + v[0] * v[1] + k[0] * k[1]]
    sols = []
    for L in solve_for_lengths(distances, cosines):
        M = [[L[i] * u[i], L[i] * v[i], L[i] * k[i]] for i in range(3)]
        sols.append(align(M, P))
    return sols, mu, mv


def p3p4(obj, img, fx, fy, cx, cy):
    """p3p::solve on 4 correspondences -> 12-list or None (no model)."""
    with np.errstate(all="ignore"):
        sols, mu, mv = p3p_all(obj, img, fx, fy, cx, cy)
    if not sols:
        return None
    X3, Y3, Z3 = (float(obj[3][j]) for j in range(3))
    best, Rt = 0.0, None
    for s, c in enumerate(sols):
        X3p = ((c[0] * X3 + c[1] * Y3) + c[2] * Z3) + c[9]
        Y3p = ((c[3] * X3 + c[4] * Y3) + c[5] * Z3) + c[10]
        Z3p = ((c[6] * X3 + c[7] * Y3) + c[8] * Z3) + c[11]
        mu3p = cx + _div(fx * X3p, Z3p)
        mv3p = cy + _div(fy * Y3p, Z3p)
        reproj = (mu3p - mu[3]) * (mu3p - mu[3]) + (mv3p - mv[3]) * (mv3p - mv[3])
        if s == 0 or best > reproj:
            best, Rt = reproj, c
    if not all(_finite(v) for v in Rt):
        return None
    return list(Rt)


# ---- EPnP
def _seq(terms):
    acc = 0.0
    for x in terms:
        acc = acc + x
    return acc


def _seqv(arr):
    """Sequential sum from 0.0 of a float64 vector (np.add.accumulate runs left to right)."""
    return float(np.add.accumulate(np.concatenate(([0.0], np.asarray(arr, np.float64))))[-1])


def control_points(S, m, cw0):
    lam, V = jacobi_sym(S)
    order = eig_order(lam, True)
    cw = [list(cw0)]
    for i in range(1, 4):
        dc = lam[order[i - 1]]
        dc = 0.0 if dc < 0 else dc
        kk = _sqrt(_div(dc, float(m)))
        cw.append([cw0[j] + kk * float(V[j, order[i - 1]]) for j in range(3)])
    CC = [[cw[j][i] - cw[0][i] for j in range(1, 4)] for i in range(3)]
    G = [[_seq(CC[r][a] * CC[r][b] for r in range(3)) for b in range(3)] for a in range(3)]
    lamg, V = jacobi_sym(G)
    lmax = lamg[0]
    lmax = lamg[1] if lamg[1] > lmax else lmax
    lmax = lamg[2] if lamg[2] > lmax else lmax
    inv = [_div(1.0, l) if l > PINV_CUT * lmax else 0.0 for l in lamg]
    W = [[_seq(float(V[a, k]) * inv[k] * float(V[b, k]) for k in range(3)) for b in range(3)] for a in range(3)]
    ci = [_seq(W[a][b] * CC[r][b] for b in range(3)) for a in range(3) for r in range(3)]
    return cw, ci


def qr_solve(A, nr, nc, b, x):
    A, b = list(A), list(b)
    A1, A2 = [0.0] * 6, [0.0] * 6
    for k in range(nc):
        eta = _abs(A[k * nc + k])
        for i in range(k + 1, nr):
            eta = _abs(A[i * nc + k]) if eta < _abs(A[i * nc + k]) else eta
        if eta == 0:
            return x
        sum2 = 0.0
        inv_eta = _div(1., eta)
        for i in range(k, nr):
            A[i * nc + k] *= inv_eta
            sum2 += A[i * nc + k] * A[i * nc + k]
        sigma = _sqrt(sum2)
        if A[k * nc + k] < 0:
            sigma = -sigma
        A[k * nc + k] += sigma
        A1[k] = sigma * A[k * nc + k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            sm = 0.0
            for i in range(k, nr):
                sm += A[i * nc + k] * A[i * nc + j]
            tau = _div(sm, A1[k])
            for i in range(k, nr):
                A[i * nc + j] -= tau * A[i * nc + k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i * nc + j] * b[i]
        tau = _div(tau, A1[j])
        for i in range(j, nr):
            b[i] -= tau * A[i * nc + j]
    x = list(x)
    x[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        sm = 0.0
        for j in range(i + 1, nc):
            sm += A[i * nc + j] * x[j]
        x[i] = _div(b[i] - sm, A2[i])
    return x


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _dist2(a, b):
    return ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2])


def l6x10_rho(v, cw):
    dv = [[[0.0] * 3 for _ in range(6)] for _ in range(4)]
    for i in range(4):
        a, b = 0, 1
        for j in range(6):
            for k in range(3):
                dv[i][j][k] = v[i][3 * a + k] - v[i][3 * b + k]
            b += 1
            if b > 3:
                a += 1
                b = a + 1
    L = []
    for i in range(6):
        d = [dv[0][i], dv[1][i], dv[2][i], dv[3][i]]
        L += [_dot3(d[0], d[0]), 2.0 * _dot3(d[0], d[1]), _dot3(d[1], d[1]), 2.0 * _dot3(d[0], d[2]), 2.0 * _dot3(d[1], d[2]),
              _dot3(d[2], d[2]), 2.0 * _dot3(d[0], d[3]), 2.0 * _dot3(d[1], d[3]), 2.0 * _dot3(d[2], d[3]), _dot3(d[3], d[3])]
    rho = [_dist2(cw[0], cw[1]), _dist2(cw[0], cw[2]), _dist2(cw[0], cw[3]), _dist2(cw[1], cw[2]), _dist2(cw[1], cw[3]), _dist2(cw[2], cw[3])]
    return L, rho


def betas_for(L, rho, which):
    nc = {1: 4, 2: 3, 3: 5}[which]
    cols = [0, 1, 3, 6] if which == 1 else list(range(nc))
    A = [L[10 * i + cols[j]] for i in range(6) for j in range(nc)]
    x = qr_solve(A, 6, nc, list(rho), [0.0] * 5)
    betas = [0.0] * 4
    if which == 1:
        if x[0] < 0:
            betas[0] = _sqrt(-x[0])
            betas[1], betas[2], betas[3] = _div(-x[1], betas[0]), _div(-x[2], betas[0]), _div(-x[3], betas[0])
        else:
            betas[0] = _sqrt(x[0])
            betas[1], betas[2], betas[3] = _div(x[1], betas[0]), _div(x[2], betas[0]), _div(x[3], betas[0])
    else:
        if x[0] < 0:
            betas[0] = _sqrt(-x[0])
            betas[1] = _sqrt(-x[2]) if x[2] < 0 else 0.0
        else:
            betas[0] = _sqrt(x[0])
            betas[1] = _sqrt(x[2]) if x[2] > 0 else 0.0
        if x[1] < 0:
            betas[0] = -betas[0]
        betas[2] = _div(x[3], betas[0]) if which == 3 else 0.0
        betas[3] = 0.0
    g = [0.0] * 4
    for _ in range(5):
        GA, gb = [], []
        for i in range(6):
            l = L[10 * i:10 * i + 10]
            GA += [((2 * l[0] * betas[0] + l[1] * betas[1]) + l[3] * betas[2]) + l[6] * betas[3],
                   ((l[1] * betas[0] + 2 * l[2] * betas[1]) + l[4] * betas[2]) + l[7] * betas[3],
                   ((l[3] * betas[0] + l[4] * betas[1]) + 2 * l[5] * betas[2]) + l[8] * betas[3],
                   ((l[6] * betas[0] + l[7] * betas[1]) + l[8] * betas[2]) + 2 * l[9] * betas[3]]
            gb.append(rho[i] - (l[0] * betas[0] * betas[0] + l[1] * betas[0] * betas[1] + l[2] * betas[1] * betas[1] + l[3] * betas[0] * betas[2] +
                                l[4] * betas[1] * betas[2] + l[5] * betas[2] * betas[2] + l[6] * betas[0] * betas[3] + l[7] * betas[1] * betas[3] +
                                l[8] * betas[2] * betas[3] + l[9] * betas[3] * betas[3]))
        g = qr_solve(GA, 6, 4, gb, g)
        betas = [betas[i] + g[i] for i in range(4)]
    return betas


def ccs_of(betas, v):
    ccs = [[0.0] * 3 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            for k in range(3):
                ccs[j][k] += betas[i] * v[i][3 * j + k]
    return ccs


def r_and_t(H, pc0, pw0):
    G = [[_seq(H[3 * r + a] * H[3 * r + b] for r in range(3)) for b in range(3)] for a in range(3)]
    lam, V = jacobi_sym(G)
    order = eig_order(lam, True)
    vv, uu = [None] * 3, [None] * 3
    for k in range(2):
        vv[k] = [float(V[i, order[k]]) for i in range(3)]
        hv = [(H[3 * i] * vv[k][0] + H[3 * i + 1] * vv[k][1]) + H[3 * i + 2] * vv[k][2] for i in range(3)]
        nn = _sqrt(_dot3(hv, hv))
        uu[k] = [_div(h, nn) for h in hv]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    vv[2], uu[2] = cross(vv[0], vv[1]), cross(uu[0], uu[1])
    R = [(uu[0][i] * vv[0][j] + uu[1][i] * vv[1][j]) + uu[2][i] * vv[2][j] for i in range(3) for j in range(3)]
    det = (((((R[0] * R[4] * R[8] + R[1] * R[5] * R[6]) + R[2] * R[3] * R[7]) - R[2] * R[4] * R[6]) - R[1] * R[3] * R[8]) - R[0] * R[5] * R[7])
    if det < 0:
        R[6], R[7], R[8] = -R[6], -R[7], -R[8]
    return R + [pc0[i] - _dot3(R[3 * i:3 * i + 3], pw0) for i in range(3)]


def epnp(obj, img, fx, fy, cx, cy):
    """solvePnP(SOLVEPNP_EPNP) on m >= 4 points (float32 [m][3], [m][2]) as the kernel's refit computes it -> 12-list."""
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
        u = (img[:, 0].astype(np.float64) - cx) * _div(1.0, fx) * fx + cx
        v = (img[:, 1].astype(np.float64) - cy) * _div(1.0, fy) * fy + cy
        M1 = np.zeros((m, 12))
        M2 = np.zeros((m, 12))
        for i in range(4):
            M1[:, 3 * i] = al[:, i] * fx
            M1[:, 3 * i + 1] = 0.0
            M1[:, 3 * i + 2] = al[:, i] * (cx - u)
            M2[:, 3 * i] = 0.0
            M2[:, 3 * i + 1] = al[:, i] * fy
            M2[:, 3 * i + 2] = al[:, i] * (cy - v)
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
            ue = cx + fx * Xc * inv_Zc
            ve = cy + fy * Yc * inv_Zc
            rep = _div(_seqv(np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))), float(m))
            res.append((rep, Rt))
    N = 0
    if res[1][0] < res[0][0]:
        N = 1
    if res[2][0] < res[N][0]:
        N = 2
    return res[N][1]


def get_subset(rng, n):
    idx = []
    for _ in range(4):
        draws = 0
        while True:
            v = rng.next() % n
            draws += 1
            if v not in idx:
                break
            if draws >= REDRAW_CAP:
                return None
        idx.append(v)
    return idx


def solve_pnp_ransac(obj, img, fx, fy, cx, cy, reprojection_error=0.4, confidence=0.98, max_iters=500):
    """-> (Rt [12] float64, mask [n] uint8, status (result, inliers, iterations, points, refit)) exactly as amos_pnp_ransac_device
    computes them for one problem whose selected points are obj (float32 [n][3]), img (float32 [n][2])."""
    obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
    n = len(obj)
    zero = np.zeros(12), np.zeros(n, np.uint8)
    if n < MODEL_POINTS:
        return zero[0], zero[1], (-1, 0, 0, n, 0)
    if n == MODEL_POINTS:
        Rt = p3p4(obj, img, fx, fy, cx, cy)
        if Rt is None:
            return zero[0], zero[1], (0, 0, 0, n, 0)
        return np.array(Rt), np.ones(n, np.uint8), (1, 4, 0, n, 0)
    thr2 = np.float32(reprojection_error * reprojection_error)
    rng = Rng()
    niters, it, max_good, best = max_iters, 0, 0, None
    while it < niters:
        idx = get_subset(rng, n)
        if idx is None:
            return zero[0], zero[1], (-2, 0, it, n, 0)
        Rt = p3p4(obj[idx], img[idx], fx, fy, cx, cy)
        if Rt is not None:
            good = int((errors(Rt, obj, img, fx, fy, cx, cy) <= thr2).sum())
            if good > max(max_good, MODEL_POINTS - 1):
                best, max_good = Rt, good
                niters = update_num_iters(confidence, _div(float(n - good), float(n)), niters)
        it += 1
    if max_good <= 0:
        return zero[0], zero[1], (0, 0, it, n, 0)
    mask = (errors(best, obj, img, fx, fy, cx, cy) <= thr2)
    ref = epnp(obj[mask], img[mask], fx, fy, cx, cy)
    ok = all(_finite(x) for x in ref)
    return np.array(ref if ok else best, np.float64), mask.astype(np.uint8), (1, max_good, it, n, 1 if ok else -1)


def rot(ax, ay, az):
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


K_TUM = (535.4, 539.2, 320.1, 247.6)


def scene(rng, n, outlier_frac=0.0, noise=0.0, R=None, t=None, planar=False, K=K_TUM):
    """A synthetic PnP problem: world points in front of the camera (float32), their float32 projections under (R, t) plus noise, gross
    outliers (20-80 px).  Returns (obj, img, true Rt [12], inlier flags)."""
    fx, fy, cx, cy = K
    R = rot(0.05, -0.08, 0.03) if R is None else R
    t = np.array([0.1, -0.05, 0.2]) if t is None else t
    Xc = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), np.full(n, 4.0) if planar else rng.uniform(2, 8, n)]
    if planar:
        Xc = Xc @ rot(0.2, 0.1, 0.0).T + np.array([0, 0, 0.5])
    X = ((Xc - t) @ R).astype(np.float32)  # world = R^T (camera - t)
    Xd = X.astype(np.float64) @ R.T + t
    img = np.c_[fx * Xd[:, 0] / Xd[:, 2] + cx, fy * Xd[:, 1] / Xd[:, 2] + cy]
    if noise:
        img = img + rng.normal(0, noise, (n, 2))
    img = img.astype(np.float32)
    inl = np.ones(n, bool)
    k = int(round(outlier_frac * n))
    if k:
        o = rng.choice(n, k, replace=False)
        img[o] += (rng.uniform(20, 80, (k, 2)) * rng.choice([-1, 1], (k, 2))).astype(np.float32)
        inl[o] = False
    return X, img, np.r_[R.reshape(9), t], inl
