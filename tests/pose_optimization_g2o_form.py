"""Optimizer::PoseOptimization in a plain form written straight from the g2o text (Optimizer.cc:363-605, optimization_algorithm_levenberg.cpp,
base_unary_edge.hpp, robust_kernel_impl.cpp, types_six_dof_expmap.cpp, se3quat.h): sums edge after edge, math.sin / cos, ** 3 and
numpy.linalg.  Independent of tests/pose_optimization_restatement.py (it shares only the edge gathering), so the two agree to rounding
amplified by the system's condition, not bit for bit."""
import math

import numpy as np

import pose_optimization_restatement as pr

DELTA = {False: float(np.float32(math.sqrt(5.991))), True: float(np.float32(math.sqrt(7.815)))}
CHI2 = {False: np.float32(5.991), True: np.float32(7.815)}


def seq_sum(terms):
    """sequential, in edge order"""
    return np.add.accumulate(terms, axis=0)[-1] if len(terms) else np.zeros(terms.shape[1:])


def quat_mul(a, b):  # x, y, z, w
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_from_matrix(R):
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0)
        w, s = 0.5 * s, 0.5 / s
        return np.array([(R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s, w])
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q = np.zeros(4)
    q[i], s = 0.5 * s, 0.5 / s
    q[3], q[j], q[k] = (R[k, j] - R[j, k]) * s, (R[j, i] + R[i, j]) * s, (R[k, i] + R[i, k]) * s
    return q


def normalized(q):
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def se3_exp(update):
    omega, upsilon = update[:3], update[3:]
    theta = np.linalg.norm(omega)
    Om = skew(omega)
    if theta < 0.00001:
        R = np.eye(3) + Om + Om @ Om
        V = R
    else:
        Om2 = Om @ Om
        R = np.eye(3) + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
        V = np.eye(3) + (1 - math.cos(theta)) / (theta * theta) * Om + (theta - math.sin(theta)) / (theta ** 3) * Om2
    return normalized(quat_from_matrix(R)), V @ upsilon


def oplus(pose, update):
    q, t = pose
    qe, te = se3_exp(update)
    return normalized(quat_mul(qe, q)), te + quat_matrix(qe) @ t


def errors(pose, cam, E):
    """-> pc [n][3], e [n][3] (third 0 for monocular), chi2 [n]"""
    q, t = pose
    pc = np.stack([E.X, E.Y, E.Z], 1) @ quat_matrix(q).T + t
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    mono = np.stack([E.u - (x / z * cam.fx + cam.cx), E.v - (y / z * cam.fy + cam.cy), np.zeros(E.n)], 1)
    invz = (1.0 / z).astype(np.float32).astype(np.float64)  # cam_project's float invz
    r0 = x * invz * cam.fx + cam.cx
    stereo = np.stack([E.u - r0, E.v - (y * invz * cam.fy + cam.cy), E.ur - (r0 - cam.bf * invz)], 1)
    e = np.where(E.stereo[:, None], stereo, mono)
    return pc, e, (e * e).sum(1) * E.w


def huber(chi2, stereo, on):
    delta = np.where(stereo, DELTA[True], DELTA[False])
    dsqr = delta * delta
    inl = (chi2 <= dsqr) | (not on)
    sq = np.sqrt(chi2)
    return np.where(inl, chi2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def jacobians(pc, cam, E):
    x, y, invz = pc[:, 0], pc[:, 1], 1.0 / pc[:, 2]
    invz2 = invz * invz
    J = np.zeros((E.n, 3, 6))
    J[:, 0, 0], J[:, 0, 1], J[:, 0, 2] = x * y * invz2 * cam.fx, -(1 + x * x * invz2) * cam.fx, y * invz * cam.fx
    J[:, 0, 3], J[:, 0, 5] = -invz * cam.fx, x * invz2 * cam.fx
    J[:, 1, 0], J[:, 1, 1], J[:, 1, 2] = (1 + y * y * invz2) * cam.fy, -x * y * invz2 * cam.fy, -x * invz * cam.fy
    J[:, 1, 4], J[:, 1, 5] = -invz * cam.fy, y * invz2 * cam.fy
    st = E.stereo
    J[st, 2, 0] = (J[:, 0, 0] - cam.bf * y * invz2)[st]
    J[st, 2, 1] = (J[:, 0, 1] + cam.bf * x * invz2)[st]
    J[st, 2, 2], J[st, 2, 3] = J[st, 0, 2], J[st, 0, 3]
    J[st, 2, 5] = (J[:, 0, 5] - cam.bf * invz2)[st]
    return J


def optimize(E, camera):
    """-> dict(ret, outlier [edges] or None, Rt [12], chi2 [edges]: the value each edge was classified by in the last round)"""
    with np.errstate(all="ignore"):
        cam = pr.Cam(camera)
        R0, t0 = camera["Rcw"].astype(np.float64).reshape(3, 3), camera["tcw"].astype(np.float64)
        if E.n < 3:
            return dict(ret=0, outlier=None, Rt=np.concatenate([R0.reshape(9), t0]), chi2=None)
        init = (normalized(quat_from_matrix(R0)), t0)
        outlier = np.zeros(E.n, bool)
        edge_chi2 = np.zeros(E.n)       # _error of every edge as computeError left it
        pose = init
        for rnd in range(4):
            pose = init
            act = ~outlier
            kernel = rnd < 3
            lam, ni, n_bad_it = 0.0, 2.0, 0
            x = np.zeros(6)
            for it in range(10 if act.any() else 0):
                pc, e, chi2 = errors(pose, cam, E)
                edge_chi2[act] = chi2[act]
                rho0, rho1 = huber(chi2, E.stereo, kernel)
                current = ini = float(seq_sum(rho0[act]))
                J = jacobians(pc, cam, E)
                H = seq_sum(np.einsum("nra,n,nrb->nab", J, rho1 * E.w, J)[act])
                b = -seq_sum((rho1[:, None] * np.einsum("nra,nr->na", J, e * E.w[:, None]))[act])
                if it == 0:
                    lam, ni, n_bad_it = 1e-5 * np.abs(np.diag(H)).max(), 2.0, 0
                rho, qmax = 0.0, 0
                while True:
                    A = H + lam * np.eye(6)
                    ok = bool(np.isfinite(A).all()) and bool((np.linalg.eigvalsh(A) >= 0).all())
                    if ok:
                        x = np.linalg.solve(A, b)
                    trial = oplus(pose, x)
                    _, _, chi2 = errors(trial, cam, E)
                    edge_chi2[act] = chi2[act]
                    temp = float(seq_sum(huber(chi2, E.stereo, kernel)[0][act])) if ok else np.finfo(np.float64).max
                    rho = (current - temp) / (float(x @ (lam * x + b)) + 1e-3)
                    if rho > 0 and np.isfinite(temp):
                        lam *= max(1.0 / 3.0, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0))
                        ni, current, pose = 2.0, temp, trial
                    else:
                        lam *= ni
                        ni *= 2
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                if qmax == 10 or rho == 0:
                    break
                n_bad_it = n_bad_it + 1 if (ini - current) * 1e3 < ini else 0
                if n_bad_it >= 3:
                    break
            _, _, chi2 = errors(pose, cam, E)
            edge_chi2[outlier] = chi2[outlier]  # an outlier edge is computed again, an inlier keeps its last error
            outlier = edge_chi2.astype(np.float32) > np.where(E.stereo, CHI2[True], CHI2[False])
            if E.n < 10:
                break
        return dict(ret=int(E.n - outlier.sum()), outlier=outlier, Rt=np.concatenate([quat_matrix(pose[0]).reshape(9), pose[1]]), chi2=edge_chi2.copy())


def pose_optimization(case):
    E, _ = pr.gather_edges(case["kps"], case["u_right"], case["match"], case["pos"], case["inv_sigma2"], case["count"])
    out = optimize(E, case["camera"])
    out["edges"] = E
    return out
