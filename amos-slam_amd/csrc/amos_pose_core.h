// amos_pose_core.h -- the arithmetic of Optimizer::PoseOptimization (Optimizer.cc:363-605) with the g2o pieces it runs
// (OptimizationAlgorithmLevenberg::solve, BaseUnaryEdge::constructQuadraticForm, RobustKernelHuber, EdgeSE3ProjectXYZOnlyPose /
// EdgeStereoSE3ProjectXYZOnlyPose, SE3Quat::exp / operator* / map, LinearSolverDense over Eigen::LDLT, Converter::toSE3Quat / toCvMat),
// restated from those sources: PARITY WITH g2o UNPINNED (g2o needs Eigen, which this project does not carry).
// Included by amos_pose.hip (device) and compilable as plain C++; tests/pose_optimization_restatement.py is the same arithmetic in Python
// floats and numpy, and the GPU tests hold the device to it bit for bit.  So every value is a double built from fm::add / sub / mul / dvd /
// sqr only (correctly rounded on both sides, nothing fused: the library builds with -ffp-contract=off), in the written order.
//
// Deviations from the reference, all deliberate:
//   (2 rho - 1)^3        two multiplications ((t t) t); the reference calls pow
//   sin / cos            sin_cos() below; the reference calls the C library
//   theta^3              (theta theta) theta in SE3Quat::exp's V; the reference calls pow
//   sums over the edges  the 21 + 6 + 1 sums of one linearisation and the one sum of a trial's chi2 are taken in the order of
//                        strided_partials() + tree_sum(): partial t of kThreads adds edges t, t + kThreads, ... (active ones only) in
//                        ascending order from 0.0, then each block of 64 partials is folded p[i] += p[i + s] for s = 32 .. 1 and the four
//                        block sums combine as (B0 + B1) + (B2 + B3).  The order depends on the edge count and kThreads alone; g2o adds
//                        edge after edge
//   SE3Quat::map         R X + t with R = toRotationMatrix(q) made once per pose; g2o rotates by the quaternion edge by edge
//   the result           R | t of the final quaternion (what SE3Quat::to_homogeneous_matrix gives), in double and rounded once to
//                        float; no second quaternion round trip
//   a failed solve       x keeps the last successful solution of the round (zero before the first); g2o's buffer is whatever the
//                        block solver allocated
//   an octave outside the table, a match index outside the frame's points: the feature is skipped and a status bit is set
//
// LDL^T (solve6): diagonal pivoting as Eigen::LDLT does it -- at step k the largest |remaining diagonal|, the lowest index on ties --
// in right-looking form.  "Not positive" (the solve fails) when any pivot is negative.  A ZERO PIVOT (|d| <= kTiny = 1 / DBL_MAX,
// Eigen's solve tolerance) is not an error: its column of L is set to zero, it updates nothing, and the solve sets that component of
// D^-1 y to zero.  A NaN pivot fails both comparisons (d < 0, |d| > kTiny) and so counts as a zero pivot: a system of NaNs solves to
// x = 0 and the trial is the pose itself.  The Python restatement follows the same rules.
//
// sin_cos(theta) for any finite theta >= 0 (theta is a norm):
//   theta >= kReduceBig (2^16): theta := theta mod fl(2 pi), exactly (fmod_: shift-and-subtract, every subtraction exact).  fl(2 pi)
//     is 2.45e-16 below 2 pi, so the argument is off by (theta / 2 pi) 2.45e-16 there: the accuracy decays linearly with theta, the
//     value is always a sine / cosine of a nearby angle.
//   k = floor(theta (2 / pi) + 0.5); r = (((theta - k P1) - k P2) - k P3) - k P4 with pi / 2 = P1 + P2 + P3 + P4 + 2e-48 (P1, P2: 33 bits, so
//     k P1 and k P2 are exact for k < 2^17): |r| <= pi / 4 + 1e-11
//   sin r = r + r z S(z), cos r = 1 + z C(z), z = r r: Taylor polynomials to r^17 / r^18 (truncation < 1e-19), Horner
//   quadrant k mod 4.
//   Worst error against the C library on the 200 001 evenly spaced points of [1e-5, 2 pi], both ends included: 1 ulp for the sine and
//   1 ulp for the cosine (kSinCosUlp; tests/test_pose_optimization_cpu.py allows one ulp more).
#pragma once

#include "amos_fmat_core.h"

namespace amos {
namespace po {

using fm::add;
using fm::dvd;
using fm::mul;
using fm::sqr;
using fm::sub;

constexpr int kThreads = 256;  // partial sums of one reduction (the device's work-group size)
constexpr int kSums = 28;      // H (21: upper triangle, row-major), b (6), chi2
constexpr int kRounds = 4, kIterations = 10, kTrials = 10;
constexpr double kDeltaMono = 2.4476518630981445;  // (double)(float)sqrt(5.991)
constexpr double kDeltaStereo = 2.7955322265625;   // (double)(float)sqrt(7.815)
constexpr float kChi2Mono = 5.991f, kChi2Stereo = 7.815f;
constexpr double kDblMax = 1.7976931348623157e308;
constexpr double kTiny = 5.562684646268003e-309;   // 1 / DBL_MAX
constexpr double kTwoOverPi = 0.6366197723675814, kTwoPi = 6.283185307179586;
constexpr double kP1 = 1.5707963267341256, kP2 = 6.077100506303966e-11, kP3 = 2.0222662487111665e-21, kP4 = 8.4784276603689e-32;
constexpr double kReduceBig = 65536.0;
constexpr double kSinCosUlp = 1.0;  // measured, see above

enum { kStatusOctave = 1, kStatusMatchIndex = 2 };  // amos_pose_result.status
enum { kActTrial = 0, kActIterate = 1, kActRoundEnd = 2 };

struct Cam { double fx, fy, cx, cy, bf; };
struct Pose { double q[4], t[3], R[9]; };             // q = x, y, z, w (unit, w >= 0); R = toRotationMatrix(q), row-major
struct Edge { float u, v, ur, X, Y, Z, w; int feat; };  // ur < 0: monocular; w = invLevelSigma2[octave]

// x mod y exactly, x >= 0, y > 0 finite: subtract y 2^e, the largest first; y 2^e <= x < 2 y 2^e makes every subtraction exact
FM_HD double fmod_(double x, double y)
{
    int ex = 0, ey = 0;
    (void)frexp(x, &ex);
    (void)frexp(y, &ey);
    for (int e = ex - ey; e >= 0; e--) {
        const double s = ldexp(y, e);
        if (x >= s) x = sub(x, s);
    }
    return x;
}


FM_HD void sin_cos(double theta, double &s, double &c)
{
    if (theta >= kReduceBig) theta = fmod_(theta, kTwoPi);
    const double k = floor(add(mul(theta, kTwoOverPi), 0.5));
    const double r = sub(sub(sub(sub(theta, mul(k, kP1)), mul(k, kP2)), mul(k, kP3)), mul(k, kP4)), z = mul(r, r);
    double ps = 1.0 / 355687428096000.0;  // 1 / 17!
    ps = add(mul(ps, z), -1.0 / 1307674368000.0);
    ps = add(mul(ps, z), 1.0 / 6227020800.0);
    ps = add(mul(ps, z), -1.0 / 39916800.0);
    ps = add(mul(ps, z), 1.0 / 362880.0);
    ps = add(mul(ps, z), -1.0 / 5040.0);
    ps = add(mul(ps, z), 1.0 / 120.0);
    ps = add(mul(ps, z), -1.0 / 6.0);
    double pc = -1.0 / 6402373705728000.0;  // -1 / 18!
    pc = add(mul(pc, z), 1.0 / 20922789888000.0);
    pc = add(mul(pc, z), -1.0 / 87178291200.0);
    pc = add(mul(pc, z), 1.0 / 479001600.0);
    pc = add(mul(pc, z), -1.0 / 3628800.0);
    pc = add(mul(pc, z), 1.0 / 40320.0);
    pc = add(mul(pc, z), -1.0 / 720.0);
    pc = add(mul(pc, z), 1.0 / 24.0);
    pc = add(mul(pc, z), -1.0 / 2.0);
    const double sr = add(r, mul(r, mul(z, ps))), cr = add(1.0, mul(z, pc));
    const int n = k == k ? (int)sub(k, mul(4.0, floor(mul(k, 0.25)))) : 0;  // k mod 4: k < 2^17, both products exact
    s = n == 0 ? sr : n == 1 ? cr : n == 2 ? -sr : -cr;
    c = n == 0 ? cr : n == 1 ? -sr : n == 2 ? -cr : sr;
}

// ---- 3 x 3 helpers, row-major; every dot product is (a0 b0 + a1 b1) + a2 b2
FM_HD double dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
    return add(add(mul(a0, b0), mul(a1, b1)), mul(a2, b2));
}
FM_HD void mat3_mul(const double *A, const double *B, double *C)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = dot3(A[i * 3], A[i * 3 + 1], A[i * 3 + 2], B[j], B[3 + j], B[6 + j]);
}

// Eigen::Quaterniond(R) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<.., 3, 3>)
FM_HD void quat_from_R(const double *R, double *q)
{
    double t = add(add(R[0], R[4]), R[8]);
    if (t > 0.0) {
        t = sqr(add(t, 1.0));
        q[3] = mul(0.5, t);
        t = dvd(0.5, t);
        q[0] = mul(sub(R[7], R[5]), t);
        q[1] = mul(sub(R[2], R[6]), t);
        q[2] = mul(sub(R[3], R[1]), t);
    } else if (R[0] >= R[4] && R[0] >= R[8]) {  // i = 0: neither m11 > m00 nor m22 > m00
        t = sqr(add(sub(sub(R[0], R[4]), R[8]), 1.0));
        q[0] = mul(0.5, t);
        t = dvd(0.5, t);
        q[3] = mul(sub(R[7], R[5]), t);
        q[1] = mul(add(R[3], R[1]), t);
        q[2] = mul(add(R[6], R[2]), t);
    } else if (R[4] > R[0] && R[4] >= R[8]) {   // i = 1
        t = sqr(add(sub(sub(R[4], R[8]), R[0]), 1.0));
        q[1] = mul(0.5, t);
        t = dvd(0.5, t);
        q[3] = mul(sub(R[2], R[6]), t);
        q[2] = mul(add(R[7], R[5]), t);
        q[0] = mul(add(R[1], R[3]), t);
    } else {                                    // i = 2
        t = sqr(add(sub(sub(R[8], R[0]), R[4]), 1.0));
        q[2] = mul(0.5, t);
        t = dvd(0.5, t);
        q[3] = mul(sub(R[3], R[1]), t);
        q[0] = mul(add(R[2], R[6]), t);
        q[1] = mul(add(R[5], R[7]), t);
    }
}

// SE3Quat::normalizeRotation: w >= 0, then unit norm (the squared norm as ((x x + y y) + z z) + w w)
FM_HD void quat_normalize(double *q)
{
    if (q[3] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqr(add(add(add(mul(q[0], q[0]), mul(q[1], q[1])), mul(q[2], q[2])), mul(q[3], q[3])));
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = dvd(q[i], n);
}

// Eigen's QuaternionBase::toRotationMatrix
FM_HD void quat_to_R(const double *q, double *R)
{
    const double tx = mul(2.0, q[0]), ty = mul(2.0, q[1]), tz = mul(2.0, q[2]);
    const double twx = mul(tx, q[3]), twy = mul(ty, q[3]), twz = mul(tz, q[3]);
    const double txx = mul(tx, q[0]), txy = mul(ty, q[0]), txz = mul(tz, q[0]);
    const double tyy = mul(ty, q[1]), tyz = mul(tz, q[1]), tzz = mul(tz, q[2]);
    R[0] = sub(1.0, add(tyy, tzz)); R[1] = sub(txy, twz); R[2] = add(txz, twy);
    R[3] = add(txy, twz); R[4] = sub(1.0, add(txx, tzz)); R[5] = sub(tyz, twx);
    R[6] = sub(txz, twy); R[7] = add(tyz, twx); R[8] = sub(1.0, add(txx, tyy));
}

// Converter::toSE3Quat: the float pose widened, SE3Quat(R, t)
FM_HD void pose_from_floats(const float *Rcw, const float *tcw, Pose &p)
{
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (double)Rcw[i];
    quat_from_R(R, p.q);
    quat_normalize(p.q);
    quat_to_R(p.q, p.R);
#pragma unroll
    for (int i = 0; i < 3; i++) p.t[i] = (double)tcw[i];
}

// VertexSE3Expmap::oplusImpl: out = SE3Quat::exp(x) * T, x = (omega, upsilon)
FM_HD void pose_update(const Pose &T, const double *x, Pose &out)
{
    const double ox = x[0], oy = x[1], oz = x[2];
    const double theta = sqr(add(add(mul(ox, ox), mul(oy, oy)), mul(oz, oz)));
    const double Om[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    double Om2[9], R[9], V[9];
    mat3_mul(Om, Om, Om2);
    if (theta < 0.00001) {
#pragma unroll
        for (int i = 0; i < 9; i++) V[i] = R[i] = add(add(i % 4 == 0 ? 1.0 : 0.0, Om[i]), Om2[i]);  // the reference's "TODO" branch, as it is
    } else {
        double s, c;
        sin_cos(theta, s, c);
        const double th2 = mul(theta, theta);
        const double a = dvd(s, theta), b = dvd(sub(1.0, c), th2), g = dvd(sub(theta, s), mul(th2, theta));
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const double id = i % 4 == 0 ? 1.0 : 0.0;
            R[i] = add(add(id, mul(a, Om[i])), mul(b, Om2[i]));
            V[i] = add(add(id, mul(b, Om[i])), mul(g, Om2[i]));
        }
    }
    double qe[4], Re[9], te[3];
    quat_from_R(R, qe);
    quat_normalize(qe);
    quat_to_R(qe, Re);
#pragma unroll
    for (int i = 0; i < 3; i++) te[i] = dot3(V[i * 3], V[i * 3 + 1], V[i * 3 + 2], x[3], x[4], x[5]);
    // SE3Quat::operator*: t = te + re * T.t, r = re * T.r, normalised
#pragma unroll
    for (int i = 0; i < 3; i++) out.t[i] = add(te[i], dot3(Re[i * 3], Re[i * 3 + 1], Re[i * 3 + 2], T.t[0], T.t[1], T.t[2]));
    const double *a = qe, *b = T.q;
    double q[4];
    q[3] = sub(sub(sub(mul(a[3], b[3]), mul(a[0], b[0])), mul(a[1], b[1])), mul(a[2], b[2]));
    q[0] = sub(add(add(mul(a[3], b[0]), mul(a[0], b[3])), mul(a[1], b[2])), mul(a[2], b[1]));
    q[1] = sub(add(add(mul(a[3], b[1]), mul(a[1], b[3])), mul(a[2], b[0])), mul(a[0], b[2]));
    q[2] = sub(add(add(mul(a[3], b[2]), mul(a[2], b[3])), mul(a[0], b[1])), mul(a[1], b[0]));
    quat_normalize(q);
#pragma unroll
    for (int i = 0; i < 4; i++) out.q[i] = q[i];
    quat_to_R(q, out.R);
}

// ---- one edge at one pose.  pc: the point in the camera frame; e: the error; returns chi2 = e^T (w I) e
FM_HD double edge_error(const Pose &T, const Cam &cam, const Edge &ed, double *pc, double *e)
{
    const double X = (double)ed.X, Y = (double)ed.Y, Z = (double)ed.Z, w = (double)ed.w;
#pragma unroll
    for (int i = 0; i < 3; i++) pc[i] = add(dot3(T.R[i * 3], T.R[i * 3 + 1], T.R[i * 3 + 2], X, Y, Z), T.t[i]);
    if (ed.ur < 0.0f) {  // EdgeSE3ProjectXYZOnlyPose: project2d, then fx, cx
        e[0] = sub((double)ed.u, add(mul(dvd(pc[0], pc[2]), cam.fx), cam.cx));
        e[1] = sub((double)ed.v, add(mul(dvd(pc[1], pc[2]), cam.fy), cam.cy));
        e[2] = 0.0;
        return add(mul(e[0], mul(w, e[0])), mul(e[1], mul(w, e[1])));
    }
    const double invz = (double)(float)dvd(1.0, pc[2]);  // EdgeStereoSE3ProjectXYZOnlyPose::cam_project: const float invz = 1.0f / z
    const double r0 = add(mul(mul(pc[0], invz), cam.fx), cam.cx);
    e[0] = sub((double)ed.u, r0);
    e[1] = sub((double)ed.v, add(mul(mul(pc[1], invz), cam.fy), cam.cy));
    e[2] = sub((double)ed.ur, sub(r0, mul(cam.bf, invz)));
    return add(add(mul(e[0], mul(w, e[0])), mul(e[1], mul(w, e[1]))), mul(e[2], mul(w, e[2])));
}

// RobustKernelHuber::robustify (rho0, rho1), or no kernel
FM_HD void robustify(double chi2, bool stereo, bool huber, double &rho0, double &rho1)
{
    const double delta = stereo ? kDeltaStereo : kDeltaMono, dsqr = mul(delta, delta);
    if (!huber || chi2 <= dsqr) { rho0 = chi2; rho1 = 1.0; return; }
    const double sqrte = sqr(chi2);
    rho0 = sub(mul(mul(2.0, sqrte), delta), dsqr);
    rho1 = dvd(delta, sqrte);
}

FM_HD double edge_robust_chi2(const Pose &T, const Cam &cam, const Edge &ed, bool huber)
{
    double pc[3], e[3], rho0, rho1;
    const double chi2 = edge_error(T, cam, ed, pc, e);
    robustify(chi2, !(ed.ur < 0.0f), huber, rho0, rho1);
    return rho0;
}

// computeError + linearizeOplus + constructQuadraticForm of one active edge, added to one partial: acc[0 .. 20] += J^T (rho1 w) J (upper
// triangle, row-major), acc[21 .. 26] -= rho1 (J^T (w e)), acc[27] += rho0
FM_HD void edge_accumulate(const Pose &T, const Cam &cam, const Edge &ed, bool huber, double *acc)
{
    double pc[3], e[3], rho0, rho1;
    const bool stereo = !(ed.ur < 0.0f);
    const double chi2 = edge_error(T, cam, ed, pc, e);
    robustify(chi2, stereo, huber, rho0, rho1);
    const double x = pc[0], y = pc[1], invz = dvd(1.0, pc[2]), invz2 = mul(invz, invz), fx = cam.fx, fy = cam.fy, w = (double)ed.w;
    double J[3][6];
    J[0][0] = mul(mul(mul(x, y), invz2), fx);
    J[0][1] = mul(-add(1.0, mul(mul(x, x), invz2)), fx);
    J[0][2] = mul(mul(y, invz), fx);
    J[0][3] = mul(-invz, fx);
    J[0][4] = 0.0;
    J[0][5] = mul(mul(x, invz2), fx);
    J[1][0] = mul(add(1.0, mul(mul(y, y), invz2)), fy);
    J[1][1] = mul(mul(mul(-x, y), invz2), fy);
    J[1][2] = mul(mul(-x, invz), fy);
    J[1][3] = 0.0;
    J[1][4] = mul(-invz, fy);
    J[1][5] = mul(mul(y, invz2), fy);
    J[2][0] = sub(J[0][0], mul(mul(cam.bf, y), invz2));
    J[2][1] = add(J[0][1], mul(mul(cam.bf, x), invz2));
    J[2][2] = J[0][2];
    J[2][3] = J[0][3];
    J[2][4] = 0.0;
    J[2][5] = sub(J[0][5], mul(cam.bf, invz2));
    const double wr = mul(rho1, w), we0 = mul(w, e[0]), we1 = mul(w, e[1]), we2 = mul(w, e[2]);
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++, k++) {
            double h = add(mul(mul(J[0][a], wr), J[0][b]), mul(mul(J[1][a], wr), J[1][b]));
            if (stereo) h = add(h, mul(mul(J[2][a], wr), J[2][b]));
            acc[k] = add(acc[k], h);
        }
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double g = add(mul(J[0][a], we0), mul(J[1][a], we1));
        if (stereo) g = add(g, mul(J[2][a], we2));
        acc[21 + a] = sub(acc[21 + a], mul(rho1, g));
    }
    acc[27] = add(acc[27], rho0);
}

// the fixed tree over kThreads partials (p is overwritten): blocks of 64 folded p[i] += p[i + s], s = 32 .. 1, then (B0 + B1) + (B2 + B3)
inline double tree_sum(double *p)
{
    for (int blk = 0; blk < kThreads; blk += 64)
        for (int s = 32; s > 0; s >>= 1)
            for (int i = 0; i < s; i++) p[blk + i] = add(p[blk + i], p[blk + i + s]);
    return add(add(p[0], p[64]), add(p[128], p[192]));
}
static_assert(kThreads == 256, "tree_sum combines four blocks of 64");

// (H + lambda I) x = b by LDL^T with diagonal pivoting (see the head of the file), in D dimensions (6: the pose; 7: the Sim3 of
// amos_sim3_opt_core.h).  H: upper triangle row-major; A (D D), y (D), perm (D): work.  Returns false, x untouched, when a pivot is negative.
template <int D>
FM_HD bool solve_ldlt(const double *H, double lambda, const double *b, double *x, double *A, double *y, int *perm)
{
    int k = 0;
    for (int i = 0; i < D; i++)
        for (int j = i; j < D; j++, k++) A[i * D + j] = A[j * D + i] = i == j ? add(H[k], lambda) : H[k];
    for (int i = 0; i < D; i++) perm[i] = i;
    bool ok = true;
    for (k = 0; k < D; k++) {
        int best = k;
        double bv = fm::fabs_(A[k * D + k]);
        for (int i = k + 1; i < D; i++) {
            const double v = fm::fabs_(A[i * D + i]);
            if (v > bv) { bv = v; best = i; }
        }
        if (best != k) {
            for (int j = 0; j < D; j++) { const double t = A[k * D + j]; A[k * D + j] = A[best * D + j]; A[best * D + j] = t; }
            for (int j = 0; j < D; j++) { const double t = A[j * D + k]; A[j * D + k] = A[j * D + best]; A[j * D + best] = t; }
            const int t = perm[k]; perm[k] = perm[best]; perm[best] = t;
        }
        const double d = A[k * D + k];
        if (d < 0.0) ok = false;
        if (fm::fabs_(d) > kTiny) {
            for (int i = k + 1; i < D; i++) A[i * D + k] = dvd(A[k * D + i], d);  // L; row k right of the diagonal keeps the column as it was
            for (int j = k + 1; j < D; j++)
                for (int i = j; i < D; i++) A[j * D + i] = A[i * D + j] = sub(A[i * D + j], mul(A[i * D + k], A[k * D + j]));
        } else {
            for (int i = k + 1; i < D; i++) A[i * D + k] = 0.0;
        }
    }
    if (!ok) return false;
    for (int i = 0; i < D; i++) y[i] = b[perm[i]];
    for (int i = 1; i < D; i++)
        for (int j = 0; j < i; j++) y[i] = sub(y[i], mul(A[i * D + j], y[j]));
    for (int i = 0; i < D; i++) y[i] = fm::fabs_(A[i * D + i]) > kTiny ? dvd(y[i], A[i * D + i]) : 0.0;
    for (int i = D - 2; i >= 0; i--)
        for (int j = i + 1; j < D; j++) y[i] = sub(y[i], mul(A[j * D + i], y[j]));
    for (int i = 0; i < D; i++) x[perm[i]] = y[i];
    return true;
}
FM_HD bool solve6(const double *H, double lambda, const double *b, double *x, double *A, double *y, int *perm)
{
    return solve_ldlt<6>(H, lambda, b, x, A, y, perm);
}

// ---- OptimizationAlgorithmLevenberg::solve as a state machine.  ONE caller (the device's lane 0, the host loop) owns the state; between
// its steps the edges are summed: lm_iteration_begin() takes the D (D + 1) / 2 + D + 1 sums at `cur`, lm_trial_done() the robust chi2 at
// `trial`.  D and the vertex type P are parameters (P needs pose_update(const P &, const double *, P &), found by its namespace); maxIter is
// optimize()'s argument.  Lm is the 6-dimension instance of PoseOptimization.
template <int D, class P>
struct LmT {
    static constexpr int kH = D * (D + 1) / 2;
    P cur, trial, lastEval;  // lastEval: where computeActiveErrors ran last (the error an inlier edge keeps into the classification)
    double H[kH], b[D], x[D], A[D * D], y[D];
    double lambda, ni, currentChi, iniChi, rho;
    int perm[D];
    int nBad, qmax, iter, trials, solved, maxIter;
};
using Lm = LmT<6, Pose>;

template <int D, class P>
FM_HD void lm_round_begin(LmT<D, P> &s, const P &init, int maxIter = kIterations)
{
    s.cur = init;
    s.lastEval = init;
    for (int i = 0; i < D; i++) s.x[i] = 0.0;
    s.lambda = 0.0; s.ni = 2.0; s.currentChi = 0.0; s.iniChi = 0.0; s.rho = 0.0;
    s.nBad = 0; s.qmax = 0; s.iter = 0; s.trials = 0; s.solved = 0; s.maxIter = maxIter;
}

template <int D, class P>
FM_HD void lm_make_trial(LmT<D, P> &s)
{
    s.solved = solve_ldlt<D>(s.H, s.lambda, s.b, s.x, s.A, s.y, s.perm) ? 1 : 0;
    pose_update(s.cur, s.x, s.trial);
}

template <int D, class P>
FM_HD void lm_iteration_begin(LmT<D, P> &s, const double *sums)
{
    constexpr int kH = LmT<D, P>::kH;
    for (int i = 0; i < kH; i++) s.H[i] = sums[i];
    for (int i = 0; i < D; i++) s.b[i] = sums[kH + i];
    s.currentChi = s.iniChi = sums[kH + D];
    s.lastEval = s.cur;
    if (s.iter == 0) {  // computeLambdaInit: tau max |H_jj|, std::max's comparisons
        double m = 0.0;
        int k = 0;
        for (int j = 0; j < D; k += D - j, j++) {
            const double a = fm::fabs_(s.H[k]);
            m = a < m ? m : a;
        }
        s.lambda = mul(1e-5, m);
        s.ni = 2.0;
        s.nBad = 0;
    }
    s.rho = 0.0;
    s.qmax = 0;
    lm_make_trial(s);
}

// -> kActTrial (s.trial is the next trial), kActIterate (linearise again at s.cur) or kActRoundEnd
template <int D, class P>
FM_HD int lm_trial_done(LmT<D, P> &s, double chiSum)
{
    const double tempChi = s.solved ? chiSum : kDblMax;
    s.lastEval = s.trial;
    double scale = 0.0;
    for (int j = 0; j < D; j++) scale = add(scale, mul(s.x[j], add(mul(s.lambda, s.x[j]), s.b[j])));
    scale = add(scale, 1e-3);
    s.rho = dvd(sub(s.currentChi, tempChi), scale);
    if (s.rho > 0.0 && sub(tempChi, tempChi) == 0.0) {  // g2o_isfinite
        const double t = sub(mul(2.0, s.rho), 1.0);
        double alpha = sub(1.0, mul(mul(t, t), t));
        alpha = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;              // std::min(alpha, _goodStepUpperScale)
        const double f = (1.0 / 3.0) < alpha ? alpha : (1.0 / 3.0);     // std::max(_goodStepLowerScale, alpha)
        s.lambda = mul(s.lambda, f);
        s.ni = 2.0;
        s.currentChi = tempChi;
        s.cur = s.trial;
    } else {
        s.lambda = mul(s.lambda, s.ni);
        s.ni = mul(s.ni, 2.0);
    }
    s.qmax++;
    s.trials++;
    if (s.rho < 0.0 && s.qmax < kTrials) {
        lm_make_trial(s);
        return kActTrial;
    }
    s.iter++;
    if (s.qmax == kTrials || s.rho == 0.0) return kActRoundEnd;
    if (mul(sub(s.iniChi, s.currentChi), 1e3) < s.iniChi) s.nBad++;
    else s.nBad = 0;
    if (s.nBad >= 3 || s.iter == s.maxIter) return kActRoundEnd;
    return kActIterate;
}

// (float) chi2 > 5.991f / 7.815f; NaN is an inlier
FM_HD bool edge_is_outlier(double chi2, bool stereo)
{
    return (float)chi2 > (stereo ? kChi2Stereo : kChi2Mono);
}

// what SetPose / UpdatePoseMatrices store
FM_HD void pose_store(const double *Rt, float *Tcw, float *Ow)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Tcw[i * 4 + j] = (float)Rt[i * 3 + j];
        Tcw[i * 4 + 3] = (float)Rt[9 + i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
        Ow[i] = (float)-dot3((double)Tcw[i], (double)Tcw[4 + i], (double)Tcw[8 + i], (double)Tcw[3], (double)Tcw[7], (double)Tcw[11]);
}

// the layout of amos_pose_result (include/amos_frontend.h)
struct Out {
    double Rt[12];
    float Tcw[12], Ow[3];
    int32_t n_edges, n_inliers, n_inliers_with_obs, rounds, status;
    int32_t iterations[4], trials[4];
    double lambda[4], chi2[4];
};

// the head of a result: everything zero but the counts and the input pose (what stands when fewer than 3 edges leave the pose untouched)
FM_HD void out_begin(Out &o, const float *Rcw, const float *tcw, int nEdges, int status)
{
    for (int i = 0; i < 9; i++) o.Rt[i] = (double)Rcw[i];
    for (int i = 0; i < 3; i++) o.Rt[9 + i] = (double)tcw[i];
    pose_store(o.Rt, o.Tcw, o.Ow);
    o.n_edges = nEdges; o.n_inliers = 0; o.n_inliers_with_obs = 0; o.rounds = 0; o.status = status;
    for (int r = 0; r < kRounds; r++) { o.iterations[r] = o.trials[r] = 0; o.lambda[r] = o.chi2[r] = 0.0; }
}
FM_HD void out_round(Out &o, int round, const Lm &s)
{
    o.rounds = round + 1;
    o.iterations[round] = s.iter; o.trials[round] = s.trials;
    o.lambda[round] = s.lambda; o.chi2[round] = s.currentChi;
    for (int i = 0; i < 9; i++) o.Rt[i] = s.cur.R[i];
    for (int i = 0; i < 3; i++) o.Rt[9 + i] = s.cur.t[i];
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One frame on the host, the device's order of operations with loops for its threads.  outlier [nEdges]: written when 3 or more edges.
// Returns nInitialCorrespondences - nBad.
inline int optimize_host(const Edge *edges, int nEdges, unsigned char *outlier, const float *Rcw, const float *tcw, const Cam &cam, int status, Out &o)
{
    out_begin(o, Rcw, tcw, nEdges, status);
    if (nEdges < 3) return 0;
    Pose init;
    pose_from_floats(Rcw, tcw, init);
    for (int e = 0; e < nEdges; e++) outlier[e] = 0;
    Lm s;
    double part[kSums][kThreads], sums[kSums];
    int nBad = 0;
    for (int round = 0; round < kRounds; round++) {
        const bool huber = round < 3;
        lm_round_begin(s, init);
        int nActive = 0;
        for (int e = 0; e < nEdges; e++) nActive += outlier[e] == 0;
        for (int act = nActive > 0 ? kActIterate : kActRoundEnd; act != kActRoundEnd;) {
            for (int t = 0; t < kThreads; t++) {
                double acc[kSums];
                for (int k = 0; k < kSums; k++) acc[k] = 0.0;
                for (int e = t; e < nEdges; e += kThreads)
                    if (!outlier[e]) edge_accumulate(s.cur, cam, edges[e], huber, acc);
                for (int k = 0; k < kSums; k++) part[k][t] = acc[k];
            }
            for (int k = 0; k < kSums; k++) sums[k] = tree_sum(part[k]);
            lm_iteration_begin(s, sums);
            do {
                for (int t = 0; t < kThreads; t++) {
                    double acc = 0.0;
                    for (int e = t; e < nEdges; e += kThreads)
                        if (!outlier[e]) acc = add(acc, edge_robust_chi2(s.trial, cam, edges[e], huber));
                    part[0][t] = acc;
                }
                act = lm_trial_done(s, tree_sum(part[0]));
            } while (act == kActTrial);
        }
        nBad = 0;
        for (int e = 0; e < nEdges; e++) {
            double pc[3], err[3];
            const double chi2 = edge_error(outlier[e] ? s.cur : s.lastEval, cam, edges[e], pc, err);
            outlier[e] = edge_is_outlier(chi2, !(edges[e].ur < 0.0f)) ? 1 : 0;
            nBad += outlier[e];
        }
        out_round(o, round, s);
        if (nEdges < 10) break;
    }
    pose_store(o.Rt, o.Tcw, o.Ow);
    o.n_inliers = nEdges - nBad;
    return o.n_inliers;
}
#endif

}  // namespace po
}  // namespace amos
