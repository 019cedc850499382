"""tests/dyna_restatement.py -- literal, loop-by-loop restatement of the tail of Tracking::GetSceneFlowObj (src/Tracking.cc:1012-1184)
and of the decision of Frame::CalDyna (src/Frame.cc:552-628), with the definitions of include/amos_frontend.h (amos_dyna_*): what
k_dyna_tail and k_dyna_decide (amos-slam_amd/csrc/amos_dyna.hip) are held to bit for bit.  Floats are numpy float32 scalars, doubles
Python floats; one rounding per written operation.  TEST INFRASTRUCTURE ONLY."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import flow_oracle as fo  # noqa: E402

f32 = np.float32
NO_PNP, NO_F2, BAD_N, RESET = 1, 2, 4, 8
BAD_MATCH_LABEL, BAD_TM_LABEL, BAD_ID = 1, 2, 4


def _gemm_row(R, r, x, y, z, t):
    """one row of a cv::Mat gemm: double accumulation left to right, one rounding"""
    return f32(((float(R[3 * r]) * float(x) + float(R[3 * r + 1]) * float(y)) + float(R[3 * r + 2]) * float(z)) + float(t))


def _sqrt32(x):
    return f32(math.sqrt(float(x)))  # correctly rounded: the double root of a float rounded to float


def world_of_last(Tlw):
    """Rwl = Rlw^T, twl = -Rlw^T tlw (Tracking.cc:970-973)"""
    T = [f32(v) for v in np.asarray(Tlw, f32).reshape(-1)]
    Rwl = [T[4 * c + r] for r in range(3) for c in range(3)]
    twl = [f32(-((float(T[r]) * float(T[3]) + float(T[4 + r]) * float(T[7])) + float(T[8 + r]) * float(T[11]))) for r in range(3)]
    return Rwl, twl


def pre3d(cam, Rwl, twl, x, y, z1):
    cx, cy, invfx, invfy = cam
    xl = f32(f32(f32(f32(x) - cx) * z1) * invfx)
    yl = f32(f32(f32(f32(y) - cy) * z1) * invfy)
    return [_gemm_row(Rwl, r, xl, yl, z1, twl[r]) for r in range(3)]


def rpe(P, X, Y, Z, u, v, fx, fy, cx, cy):
    """cv::projectPoints with R itself (no Rodrigues round trip): doubles, z ? 1 / z : 1, u, v as float; Rpe = sqrtf(du^2 + dv^2)"""
    P = [float(p) for p in P]
    X, Y, Z = float(X), float(Y), float(Z)
    xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3]
    yc = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7]
    zc = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11]
    iz = 1.0 / zc if zc != 0.0 else 1.0
    uu = f32((xc * iz) * fx + cx)
    vv = f32((yc * iz) * fy + cy)
    du, dv = f32(f32(u) - uu), f32(f32(v) - vv)
    return _sqrt32(f32(f32(du * du) + f32(dv * dv)))


def set_pose(P):
    """Frame::SetPose: Rwc = Rcw^T, Ow = -Rcw^T tcw (one gemm: double accumulation, one rounding)"""
    P = [f32(p) for p in P]
    Rwc = [P[4 * c + r] for r in range(3) for c in range(3)]
    Ow = [f32(-((float(P[r]) * float(P[3]) + float(P[4 + r]) * float(P[7])) + float(P[8 + r]) * float(P[11]))) for r in range(3)]
    return Rwc, Ow


def _depth(d, x, y):
    h, w = d.shape
    ix, iy = int(x), int(y)
    if not (x >= 0 and y >= 0 and ix < w and iy < h):
        return f32(0)
    return f32(d[iy, ix])


def tail(pre, nxt, state, n, F2, fmat_status, Rt, pnp_status, depth_last, depth_cur, cam, Tlw, fx, fy, motion, lk=None, max_points=4096):
    """Tracking.cc:1012-1184 as amos_dyna_tail_device defines it.  cam = (cx, cy, invfx, invfy) floats; Rt: 12 doubles (R row-major, t);
    motion / lk: rows of [R | t].  Returns a dict shaped like SceneFlowDyna.fetch()."""
    status = (NO_PNP if pnp_status[0] != 1 else 0) | (NO_F2 if fmat_status[4] != 1 else 0)
    if n < 0 or n > max_points:
        return dict(counts=np.zeros(6, np.int32), pose=np.zeros(12, f32), rwc=np.zeros(9, f32), ow=np.zeros(3, f32), choice=0, status=status | BAD_N,
                    match=np.zeros((0, 2), f32), rpe=np.zeros(0, f32), epipolar=np.zeros(0), tm=np.zeros((0, 2), f32), flow=np.zeros((0, 3), f32))
    cam = tuple(f32(c) for c in cam)
    cx, cy = float(cam[0]), float(cam[1])
    Rwl, twl = world_of_last(Tlw)
    Rt = [float(v) for v in Rt]
    Mod = [f32(Rt[3 * r + c]) if c < 3 else f32(Rt[9 + r]) for r in range(3) for c in range(4)]
    motion = [f32(v) for v in np.asarray(motion, f32).reshape(-1)]
    score = [f32(v) for v in np.asarray(lk, f32).reshape(-1)] if lk is not None else Mod
    # the reference's lists over state != 0 (Tracking.cc:955-990)
    match_pre = [pre[i] for i in range(n) if state[i] != 0]
    match_cur = [nxt[i] for i in range(n) if state[i] != 0]
    pre_3d, cur_2d, zs = [], [], []
    for p, q in zip(match_pre, match_cur):
        z1, z2 = _depth(depth_last, p[0], p[1]), _depth(depth_cur, q[0], q[1])
        zs.append((z1, z2))
        if z1 > 0 and z2 > 0:
            pre_3d.append(pre3d(cam, Rwl, twl, p[0], p[1], z1))
            cur_2d.append((f32(q[0]), f32(q[1])))
        else:
            pre_3d.append([f32(0), f32(0), f32(0)])
            cur_2d.append((f32(0), f32(0)))
    mvMatch, RpePNP, RpeMotion = [], [], []
    pnp_in = mm_in = 0
    for i in range(len(pre_3d)):  # loop 1
        if pre_3d[i][2] > 0 and (cur_2d[i][0] != 0 and cur_2d[i][1] != 0):
            e = rpe(score, *pre_3d[i], *cur_2d[i], fx, fy, cx, cy)
            mvMatch.append(cur_2d[i])
            RpePNP.append(e)
            if float(e) <= 0.4:
                pnp_in += 1
    for i in range(len(pre_3d)):  # loop 2
        if pre_3d[i][2] > 0 and (cur_2d[i][0] != 0 and cur_2d[i][1] != 0):
            e = rpe(motion, *pre_3d[i], *cur_2d[i], fx, fy, cx, cy)
            RpeMotion.append(e)
            if float(e) <= 0.4:
                mm_in += 1
    if pnp_in >= mm_in:
        output, mvRpe, choice = Mod, RpePNP, 1
    else:
        output, mvRpe, choice = motion, RpeMotion, 0
    Rwc, Ow = set_pose(output)
    with np.errstate(divide="ignore", invalid="ignore"):
        dd = fo.epipolar(F2, np.asarray(pre, f32)[:n].reshape(-1, 2), np.asarray(nxt, f32)[:n].reshape(-1, 2))
    mvepipolar = np.zeros(n)
    T_M = []
    for i in range(n):
        if state[i] != 0:
            mvepipolar[i] = dd[i]
            if dd[i] <= 1:
                continue
            T_M.append((f32(nxt[i][0]), f32(nxt[i][1])))
    vFlow = []
    for i in range(len(match_cur)):
        z1, z2 = zs[i]
        if z1 > 0 and z2 > 0:
            p = pre3d(cam, Rwl, twl, match_pre[i][0], match_pre[i][1], z1)
            xc = f32(f32(f32(f32(match_cur[i][0]) - cam[0]) * z1) * cam[2])
            yc = f32(f32(f32(f32(match_cur[i][1]) - cam[1]) * z1) * cam[3])
            c0, c2 = _gemm_row(Rwc, 0, xc, yc, z2, Ow[0]), _gemm_row(Rwc, 2, xc, yc, z2, Ow[2])
            dx, dz = f32(p[0] - c0), f32(p[2] - c2)
            sf = _sqrt32(f32(f32(dx * dx) + f32(dz * dz)))
            if sf > 3:
                vFlow.append((f32(match_cur[i][0]), f32(match_cur[i][1]), sf))
    counts = np.array([len(match_cur), len(mvMatch), pnp_in, mm_in, len(T_M), len(vFlow)], np.int32)
    return dict(counts=counts, pose=np.array(output, f32), rwc=np.array(Rwc, f32), ow=np.array(Ow, f32), choice=choice, status=status,
                match=np.array(mvMatch, f32).reshape(-1, 2), rpe=np.array(mvRpe, f32), epipolar=mvepipolar, tm=np.array(T_M, f32).reshape(-1, 2),
                flow=np.array(vFlow, f32).reshape(-1, 3))


def reset():
    """the first frame (Tracking.cc:377): GetSceneFlowObj is not called, the lists are empty"""
    return dict(counts=np.zeros(6, np.int32), pose=np.zeros(12, f32), rwc=np.zeros(9, f32), ow=np.zeros(3, f32), choice=0, status=RESET,
                match=np.zeros((0, 2), f32), rpe=np.zeros(0, f32), epipolar=np.zeros(0), tm=np.zeros((0, 2), f32), flow=np.zeros((0, 3), f32))


def _label(labels, n_centers, x, y):
    h, w = labels.shape
    ix, iy = int(x), int(y)
    if not (x >= 0 and y >= 0 and ix < w and iy < h):
        return 0
    v = float(labels[iy, ix])
    return int(v) if 1.0 <= v <= float(n_centers) else 0


def decide(match, rpe_list, tm, labels, center_ids, k):
    """Frame.cc:552-628 as amos_dyna_decide_batch_device defines it: (rm [k] int32, AveClusterRpe [k] float32, epNum [k] int32, status)."""
    n_centers = len(center_ids)
    status = 0
    clusterRpe = [[] for _ in range(k)]
    for i in range(len(match)):
        pixelId = _label(labels, n_centers, match[i][0], match[i][1])
        if pixelId == 0:
            status |= BAD_MATCH_LABEL
            continue
        cid = int(center_ids[pixelId - 1])
        if not 0 <= cid < k:
            status |= BAD_ID
            continue
        clusterRpe[cid].append(f32(rpe_list[i]))
    ave = np.zeros(k, f32)
    for i in range(k):
        s = f32(0)
        for r in clusterRpe[i]:
            s = f32(s + r)
        with np.errstate(invalid="ignore", divide="ignore"):
            ave[i] = f32(s / f32(len(clusterRpe[i])))  # an empty cluster: 0 / 0 = NaN
    labelset = set()
    for i in range(len(tm)):
        lab = _label(labels, n_centers, tm[i][0], tm[i][1])
        if lab == 0:
            status |= BAD_TM_LABEL
            continue
        labelset.add(lab)
    ep = np.zeros(k, np.int32)
    for lab in sorted(labelset):
        cid = int(center_ids[lab - 1])
        if not 0 <= cid < k:
            status |= BAD_ID
            continue
        ep[cid] += 1
    rm = np.array([1 if ep[i] > 0 and ave[i] >= 3 else 0 for i in range(k)], np.int32)
    return rm, ave, ep, status


# ---- synthetic inputs shared by the CPU and GPU tests
CAM = (f32(320.1), f32(247.6), f32(1 / 535.4), f32(1 / 539.2))
FX, FY = float(f32(535.4)), float(f32(539.2))


def small_pose(rng, rot=0.01, trans=0.05):
    a = rng.normal(0, rot, 3)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + K + 0.5 * K @ K  # near a rotation; exactness does not matter
    t = rng.normal(0, trans, 3)
    return np.c_[R, t].astype(f32)


def project(P, X):
    P = np.asarray(P, np.float64).reshape(3, 4)
    c = P[:, :3] @ np.asarray(X, np.float64).T + P[:, 3:4]
    cx, cy, ifx, ify = (float(v) for v in CAM)
    return np.c_[c[0] / c[2] * FX + cx, c[1] / c[2] * FY + cy]


def scene(rng, n, moving=0.2, noise=0.05, holes=0.05, state_p=0.9, Tlw=None, far_band=True):
    """n tracked points: pre / next pairs consistent with a pose T (plus `moving` of them displaced), depth maps with holes, a state mix.
    far_band: a band of the current depth map 4 m farther (scene flow above 3 there).  Returns dict(pre, nxt, state, depth_last, depth_cur, Tlw, T)."""
    Tlw = np.eye(3, 4, dtype=f32) if Tlw is None else np.asarray(Tlw, f32)
    yy, xx = np.mgrid[0:480, 0:640]
    depth_last = (2.0 + 0.5 * np.sin(xx / 90.0) * np.cos(yy / 70.0)).astype(f32)
    depth_last[rng.random(depth_last.shape) < holes] = 0
    depth_cur = depth_last.copy()
    depth_cur[rng.random(depth_cur.shape) < holes] = 0
    if far_band:
        depth_cur[:, 400:480] += np.where(depth_cur[:, 400:480] > 0, f32(4.0), f32(0.0))
    pre = np.c_[rng.uniform(6, 633, n), rng.uniform(6, 473, n)].astype(f32)
    T = small_pose(rng)
    Rwl, twl = world_of_last(Tlw)
    X = np.array([pre3d(CAM, Rwl, twl, p[0], p[1], f32(max(depth_last[int(p[1]), int(p[0])], f32(1.0)))) for p in pre], np.float64).reshape(-1, 3)
    nxt = project(T, X) + rng.normal(0, noise, (n, 2))
    mv = rng.random(n) < moving
    nxt[mv] += rng.uniform(8, 20, (int(mv.sum()), 2))
    nxt = np.clip(nxt, 6, [633, 473]).astype(f32)
    state = (rng.random(n) < state_p).astype(np.uint8)
    return dict(pre=pre, nxt=nxt, state=state, depth_last=depth_last, depth_cur=depth_cur, Tlw=Tlw, T=T)


def fundamental_of(T):
    """F = K^-T [t]x R K^-1 of a pose (float64, last entry 1 where possible)"""
    T = np.asarray(T, np.float64).reshape(3, 4)
    cx, cy = float(CAM[0]), float(CAM[1])
    K = np.array([[FX, 0, cx], [0, FY, cy], [0, 0, 1.0]])
    t = T[:, 3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ T[:, :3] @ Ki
    return (F / F[2, 2] if abs(F[2, 2]) > 1e-12 else F).reshape(9)


def rt_of(P):
    """a 3 x 4 float pose as the 12 doubles of amos_pnp's R | t"""
    P = np.asarray(P, np.float64).reshape(3, 4)
    return np.r_[P[:, :3].reshape(-1), P[:, 3]]
