// amos_sim3_opt_core.h -- the arithmetic of Optimizer::OptimizeSim3 (Optimizer.cc:1364-1590) with the g2o pieces it runs (VertexSim3Expmap::
// oplusImpl, Sim3(const Vector7d &) / operator* / inverse / map of sim3.h, EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError,
// BaseBinaryEdge::linearizeOplus -- the numeric central difference, because both edges have their own linearizeOplus commented out --,
// BaseBinaryEdge::constructQuadraticForm, RobustKernelHuber, OptimizationAlgorithmLevenberg::solve, LinearSolverDense over Eigen::LDLT,
// Converter::toCvMat(g2o::Sim3)), restated from those sources: PARITY WITH g2o UNPINNED (g2o needs Eigen, which this
// project does not carry).  Included by amos_sim3_opt.hip (device) and compilable as plain C++; tests/sim3_optimization_restatement.py is the
// same arithmetic in Python floats and numpy, and the tests hold both compilations to it bit for bit.  So every value is a double built from
// fm::add / sub / mul / dvd / sqr only (correctly rounded on both sides, nothing fused), in the written order.  The Levenberg state machine,
// the LDL^T solve, sin_cos, the quaternion helpers and the reduction tree are amos_pose_core.h's (po::LmT<7, Pose>, po::solve_ldlt<7>).
//
// Deviations from the reference, all deliberate:
//   sin / cos            po::sin_cos; the reference calls the C library
//   exp(sigma)           exp_() below; the reference calls the C library
//   Sim3::map            (s R) X + t with sR = s * toRotationMatrix(r) made once per pose, for the estimate and for its inverse(); g2o
//                        rotates by the quaternion edge by edge, scales afterwards, and inverts the estimate edge by edge
//   Sim3::operator*      the translation s (R t') + t with R = toRotationMatrix(r) of the left factor; g2o rotates by the quaternion
//   Sim3::inverse        the translation R(conj r) ((-1 / s) t) by the matrix of the conjugate
//   the 14 perturbed estimates of one linearisation (oplus(+-delta e_d), d = 0 .. 6) and their inverses depend on the estimate alone and
//                        are made once per linearisation, from 14 updates Sim3(+-delta e_d) made once per call (update_make /
//                        update_apply: the same operations as one oplus); g2o makes them edge by edge (push / oplus / pop)
//   sums over the edges  the 28 + 7 + 1 sums of one linearisation and the one sum of a trial's chi2 are taken in the order of
//                        po's strided_partials() + tree_sum(): partial t of kThreads takes the ACTIVE correspondences c = t, t + kThreads, ...
//                        in ascending order from 0.0 and adds for each the term of e12 (EdgeSim3ProjectXYZ), then the term of e21
//                        (EdgeInverseSim3ProjectXYZ); the partials fold as po::tree_sum.  The order depends on the correspondence count
//                        and kThreads alone; g2o adds edge after edge
//   a failed solve       x keeps the last successful solution of the round (zero before the first), as in amos_pose_core.h
//   the result           R12 = toRotationMatrix(r) of the final quaternion (NOT normalised: g2o's Sim3 never normalises), t12, s12 each
//                        rounded once to float; when the function returns 0 ahead of the second optimisation the record carries the
//                        input floats as they came
//   an octave outside the table, a row entry outside keyframe 2: the feature is skipped; the octave sets a status bit
//
// exp_(x):  k = floor(x / ln 2 + 0.5);  r = (x - k L1) - k L2 with ln 2 = L1 + L2 (L1: 32 bits, k L1 exact for |k| < 2^20): |r| <= 0.3466;
//   e^r by the Taylor polynomial to r^13 (truncation < 5e-18), Horner from 1 / 13! down to 1 + r (...); ldexp(., k).  exp_(0.0) == 1.0
//   exactly (k = 0, r = 0, every Horner step gives its constant): fix_scale rests on it.  |x| > 800 is clamped (0 / infinity), NaN stays.
//   Worst error against the C library on the 200 001 evenly spaced points of [-1, 1] plus +-1e-9: 1 ulp (kExpUlp;
//   tests/test_sim3_optimization_cpu.py allows one ulp more).
#pragma once

#include "amos_pose_core.h"

namespace amos {
namespace so {

using fm::add;
using fm::dvd;
using fm::mul;
using fm::sqr;
using fm::sub;

constexpr int kThreads = po::kThreads;
constexpr int kDim = 7, kH = 28, kSums = 36;  // H (28: upper triangle, row-major), b (7), chi2
constexpr int kFirstIterations = 5, kMoreIterationsBad = 10, kMoreIterationsClean = 5, kMinCorrespondences = 10;
constexpr double kDelta = 1e-9, kScalar = 1.0 / (2 * 1e-9);  // base_binary_edge.hpp:147-148
constexpr double kEps = 0.00001;                             // sim3.h:90
constexpr double kLn2Hi = 6.93147180369123816490e-01, kLn2Lo = 1.90821492927058770002e-10, kInvLn2 = 1.44269504088896338700e+00;
constexpr double kExpUlp = 1.0;  // measured, see above

enum { kStatusOctave = 1 };  // amos_sim3_opt_result.status

struct Map { double sR[9], t[3]; };  // X -> sR X + t
struct Pose {                        // g2o::Sim3: r = x, y, z, w (not normalised), t, s; with the two maps every edge reads
    double q[4], t[3], s;
    Map fwd, inv;                    // the estimate's map, its inverse()'s map
    int fixScale, pad;
};
struct Cams { double k1[4], k2[4]; };  // fx, fy, cx, cy of keyframe 1 and keyframe 2
struct Corr {                          // one correspondence: 56 bytes
    float P1[3], P2[3];                // P3D1c, P3D2c
    float o1[2], o2[2];                // mvKeysUn[i].pt, mvKeysUn[j].pt
    float w1, w2;                      // invLevelSigma2 of each keypoint's octave
    int feat, j;
};

// The device reads the 15 estimates of a linearisation from LDS column by column of the Jacobian: read ahead of the edge loop (which the
// compiler does when it may) they would take 720 registers.  A compiler-level fence, no instruction.
#if defined(__HIP_DEVICE_COMPILE__)
#define SO_READ_HERE() asm volatile("" ::: "memory")
#else
#define SO_READ_HERE() ((void)0)
#endif

FM_HD double exp_(double x)
{
    if (x != x) return x;
    if (x > 800.0) x = 800.0;
    if (x < -800.0) x = -800.0;
    const double k = floor(add(mul(x, kInvLn2), 0.5));
    const double r = sub(sub(x, mul(k, kLn2Hi)), mul(k, kLn2Lo));
    double p = 1.0 / 6227020800.0;  // 1 / 13!
    p = add(mul(p, r), 1.0 / 479001600.0);
    p = add(mul(p, r), 1.0 / 39916800.0);
    p = add(mul(p, r), 1.0 / 3628800.0);
    p = add(mul(p, r), 1.0 / 362880.0);
    p = add(mul(p, r), 1.0 / 40320.0);
    p = add(mul(p, r), 1.0 / 5040.0);
    p = add(mul(p, r), 1.0 / 720.0);
    p = add(mul(p, r), 1.0 / 120.0);
    p = add(mul(p, r), 1.0 / 24.0);
    p = add(mul(p, r), 1.0 / 6.0);
    p = add(mul(p, r), 0.5);
    p = add(mul(p, r), 1.0);
    p = add(mul(p, r), 1.0);
    return ldexp(p, (int)k);
}

// Eigen's quaternion product a * b
FM_HD void quat_mul(const double *a, const double *b, double *q)
{
    q[3] = sub(sub(sub(mul(a[3], b[3]), mul(a[0], b[0])), mul(a[1], b[1])), mul(a[2], b[2]));
    q[0] = sub(add(add(mul(a[3], b[0]), mul(a[0], b[3])), mul(a[1], b[2])), mul(a[2], b[1]));
    q[1] = sub(add(add(mul(a[3], b[1]), mul(a[1], b[3])), mul(a[2], b[0])), mul(a[0], b[2]));
    q[2] = sub(add(add(mul(a[3], b[2]), mul(a[2], b[3])), mul(a[0], b[1])), mul(a[1], b[0]));
}

// the two maps of an estimate (q, t, s are set)
FM_HD void pose_finish(Pose &p)
{
    double R[9];
    po::quat_to_R(p.q, R);
#pragma unroll
    for (int i = 0; i < 9; i++) p.fwd.sR[i] = mul(p.s, R[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) p.fwd.t[i] = p.t[i];
    // inverse(): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    const double qi[4] = {-p.q[0], -p.q[1], -p.q[2], p.q[3]};
    po::quat_to_R(qi, R);
    const double si = dvd(1.0, p.s), ms = dvd(-1.0, p.s);
    const double u0 = mul(ms, p.t[0]), u1 = mul(ms, p.t[1]), u2 = mul(ms, p.t[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) p.inv.t[i] = po::dot3(R[i * 3], R[i * 3 + 1], R[i * 3 + 2], u0, u1, u2);
#pragma unroll
    for (int i = 0; i < 9; i++) p.inv.sR[i] = mul(si, R[i]);
}

// Sim3(Matrix3d R, Vector3d t, double s) from the float R12, t12, s12 widened: r = Quaterniond(R), not normalised
FM_HD void pose_from_floats(const float *R12, const float *t12, float s12, int fixScale, Pose &p)
{
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (double)R12[i];
    po::quat_from_R(R, p.q);
#pragma unroll
    for (int i = 0; i < 3; i++) p.t[i] = (double)t12[i];
    p.s = (double)s12;
    p.fixScale = fixScale;
    p.pad = 0;
    pose_finish(p);
}

// Sim3(const Vector7d &update) (sim3.h:70-142): x = (omega, upsilon, sigma), sigma = 0 under fix_scale.  It depends on x alone, so the 14
// updates of the numeric Jacobian are made once per call.
struct Update { double q[4], R[9], t[3], s; };  // r, toRotationMatrix(r), t, s
FM_HD void update_make(const double *x, int fixScale, Update &u)
{
    const double ox = x[0], oy = x[1], oz = x[2], sigma = fixScale ? 0.0 : x[6];
    const double theta = sqr(add(add(mul(ox, ox), mul(oy, oy)), mul(oz, oz)));
    const double Om[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    double Om2[9], R[9];
    po::mat3_mul(Om, Om, Om2);
    const double s = exp_(sigma);
    const bool smallS = fm::fabs_(sigma) < kEps, smallT = theta < kEps;
    double sn = 0.0, cs = 1.0, A, B, C;
    if (smallT) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = add(add(i % 4 == 0 ? 1.0 : 0.0, Om[i]), Om2[i]);
    } else {
        po::sin_cos(theta, sn, cs);
        const double a = dvd(sn, theta), b = dvd(sub(1.0, cs), mul(theta, theta));
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = add(add(i % 4 == 0 ? 1.0 : 0.0, mul(a, Om[i])), mul(b, Om2[i]));
    }
    if (smallS) {
        C = 1.0;
        if (smallT) {
            A = 1.0 / 2.0;
            B = 1.0 / 6.0;
        } else {
            const double theta2 = mul(theta, theta);
            A = dvd(sub(1.0, cs), theta2);
            B = dvd(sub(theta, sn), mul(theta2, theta));
        }
    } else {
        C = dvd(sub(s, 1.0), sigma);
        if (smallT) {
            const double sigma2 = mul(sigma, sigma);
            A = dvd(add(mul(sub(sigma, 1.0), s), 1.0), sigma2);
            B = dvd(mul(add(sub(mul(0.5, sigma2), sigma), 1.0), s), mul(sigma2, sigma));
        } else {
            const double a = mul(s, sn), b = mul(s, cs), theta2 = mul(theta, theta), sigma2 = mul(sigma, sigma), c = add(theta2, sigma2);
            A = dvd(add(mul(a, sigma), mul(sub(1.0, b), theta)), mul(theta, c));
            B = dvd(sub(C, dvd(add(mul(sub(b, 1.0), sigma), mul(a, theta)), c)), theta2);
        }
    }
    po::quat_from_R(R, u.q);
    po::quat_to_R(u.q, u.R);
    u.s = s;
#pragma unroll
    for (int i = 0; i < 3; i++) {  // t = W upsilon, W = A Omega + B Omega2 + C I
        const double w0 = add(add(mul(A, Om[i * 3]), mul(B, Om2[i * 3])), mul(C, i == 0 ? 1.0 : 0.0));
        const double w1 = add(add(mul(A, Om[i * 3 + 1]), mul(B, Om2[i * 3 + 1])), mul(C, i == 1 ? 1.0 : 0.0));
        const double w2 = add(add(mul(A, Om[i * 3 + 2]), mul(B, Om2[i * 3 + 2])), mul(C, i == 2 ? 1.0 : 0.0));
        u.t[i] = po::dot3(w0, w1, w2, x[3], x[4], x[5]);
    }
}

// Sim3::operator* (sim3.h:266-272): out = u * T: r = u.r * T.r, t = u.s (u.r * T.t) + u.t, s = u.s * T.s
FM_HD void update_apply(const Update &u, const Pose &T, Pose &out)
{
    double q[4], t[3];
    quat_mul(u.q, T.q, q);
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = add(mul(u.s, po::dot3(u.R[i * 3], u.R[i * 3 + 1], u.R[i * 3 + 2], T.t[0], T.t[1], T.t[2])), u.t[i]);
    const double s = mul(u.s, T.s);
    const int fixScale = T.fixScale;
#pragma unroll
    for (int i = 0; i < 4; i++) out.q[i] = q[i];
#pragma unroll
    for (int i = 0; i < 3; i++) out.t[i] = t[i];
    out.s = s;
    out.fixScale = fixScale;
    out.pad = 0;
    pose_finish(out);
}

// VertexSim3Expmap::oplusImpl: out = Sim3(x) * T
FM_HD void pose_update(const Pose &T, const double *x, Pose &out)
{
    Update u;
    update_make(x, T.fixScale, u);
    update_apply(u, T, out);
}

// the update by +delta (k even) or -delta (k odd) along e_(k / 2): the 14 updates of the numeric linearisation
FM_HD void perturbation(int k, int fixScale, Update &u)
{
    double x[kDim];
#pragma unroll
    for (int d = 0; d < kDim; d++) x[d] = d == (k >> 1) ? ((k & 1) ? -kDelta : kDelta) : 0.0;
    update_make(x, fixScale, u);
}

// computeError of one edge at one map: e = obs - cam_map(project(M X)); returns chi2 = e^T (w I) e
FM_HD double edge_error(const Map &M, const double *K, const float *Xf, const float *obs, double w, double *e)
{
    const double X = (double)Xf[0], Y = (double)Xf[1], Z = (double)Xf[2];
    const double p0 = add(po::dot3(M.sR[0], M.sR[1], M.sR[2], X, Y, Z), M.t[0]);
    const double p1 = add(po::dot3(M.sR[3], M.sR[4], M.sR[5], X, Y, Z), M.t[1]);
    const double p2 = add(po::dot3(M.sR[6], M.sR[7], M.sR[8], X, Y, Z), M.t[2]);
    e[0] = sub((double)obs[0], add(mul(dvd(p0, p2), K[0]), K[2]));
    e[1] = sub((double)obs[1], add(mul(dvd(p1, p2), K[1]), K[3]));
    return add(mul(e[0], mul(w, e[0])), mul(e[1], mul(w, e[1])));
}

// (double)(float) sqrt(th2): Optimizer.cc:1424
FM_HD double huber_delta(float th2) { return (double)(float)sqr((double)th2); }

// RobustKernelHuber::robustify (rho0, rho1)
FM_HD void robustify(double chi2, double delta, double &rho0, double &rho1)
{
    const double dsqr = mul(delta, delta);
    if (chi2 <= dsqr) { rho0 = chi2; rho1 = 1.0; return; }
    const double sqrte = sqr(chi2);
    rho0 = sub(mul(mul(2.0, sqrte), delta), dsqr);
    rho1 = dvd(delta, sqrte);
}

// computeError + the numeric linearizeOplus + constructQuadraticForm of one edge, added to one partial: acc[0 .. 27] += J^T (rho1 w) J (upper
// triangle, row-major), acc[28 .. 34] -= rho1 (J^T (w e)), acc[35] += rho0, sum k at acc[k * S] (the device keeps its partials in LDS, one
// column per thread).  pert: the estimate behind each of the 14 perturbation()s.
template <int S>
FM_HD void edge_accumulate(const Pose &cur, const Pose *pert, bool inverse, const double *K, const float *X, const float *obs, double w, double delta,
                           double *acc)
{
    double e[2], rho0, rho1, J[2][kDim];
    const double chi2 = edge_error(inverse ? cur.inv : cur.fwd, K, X, obs, w, e);
    robustify(chi2, delta, rho0, rho1);
#pragma unroll
    for (int d = 0; d < kDim; d++) {
        double ep[2], em[2];
        SO_READ_HERE();
        edge_error(inverse ? pert[2 * d].inv : pert[2 * d].fwd, K, X, obs, w, ep);
        edge_error(inverse ? pert[2 * d + 1].inv : pert[2 * d + 1].fwd, K, X, obs, w, em);
        J[0][d] = mul(kScalar, sub(ep[0], em[0]));
        J[1][d] = mul(kScalar, sub(ep[1], em[1]));
    }
    const double wr = mul(rho1, w), we0 = mul(w, e[0]), we1 = mul(w, e[1]);
    int k = 0;
#pragma unroll
    for (int a = 0; a < kDim; a++)
#pragma unroll
        for (int b = a; b < kDim; b++, k++) acc[k * S] = add(acc[k * S], add(mul(mul(J[0][a], wr), J[0][b]), mul(mul(J[1][a], wr), J[1][b])));
#pragma unroll
    for (int a = 0; a < kDim; a++) acc[(kH + a) * S] = sub(acc[(kH + a) * S], mul(rho1, add(mul(J[0][a], we0), mul(J[1][a], we1))));
    acc[(kH + kDim) * S] = add(acc[(kH + kDim) * S], rho0);
}

// one active correspondence in one partial: e12 (KF2's point through S12 into KF1), then e21 (KF1's point through S12^-1 into KF2)
template <int S>
FM_HD void corr_accumulate(const Pose &cur, const Pose *pert, const Cams &cams, const Corr &c, double delta, double *acc)
{
    edge_accumulate<S>(cur, pert, false, cams.k1, c.P2, c.o1, (double)c.w1, delta, acc);
    edge_accumulate<S>(cur, pert, true, cams.k2, c.P1, c.o2, (double)c.w2, delta, acc);
}

// acc + rho0(e12) + rho0(e21) at one estimate
FM_HD double corr_robust_chi2(const Pose &T, const Cams &cams, const Corr &c, double delta, double acc)
{
    double e[2], rho0, rho1;
    robustify(edge_error(T.fwd, cams.k1, c.P2, c.o1, (double)c.w1, e), delta, rho0, rho1);
    acc = add(acc, rho0);
    robustify(edge_error(T.inv, cams.k2, c.P1, c.o2, (double)c.w2, e), delta, rho0, rho1);
    return add(acc, rho0);
}

// e12->chi2() > th2 || e21->chi2() > th2 in double; NaN is an inlier
FM_HD bool corr_is_bad(const Pose &T, const Cams &cams, const Corr &c, float th2)
{
    double e[2];
    const double c12 = edge_error(T.fwd, cams.k1, c.P2, c.o1, (double)c.w1, e), c21 = edge_error(T.inv, cams.k2, c.P1, c.o2, (double)c.w2, e);
    return c12 > (double)th2 || c21 > (double)th2;
}

// the layout of amos_sim3_opt_result (include/amos_frontend.h)
struct Out {
    double q[4], t[3], s;
    double lambda[2], chi2[2];
    float R12[9], t12[3], s12, Scw[16];
    int32_t n_correspondences, n_bad_first, n_inliers, rounds;
    int32_t iterations[2], trials[2];
    int32_t status, skipped, code;
};

// Scw = gScm * Sim3(R2w, t2w, 1.0) as Converter::toCvMat(g2o::Sim3) stores it (LoopClosing.cc:470-473): [s R | t] over 0 0 0 1, float
FM_HD void scw_store(const Pose &p, const float *R2w, const float *t2w, float *Scw)
{
    double R[9], q2[4], q[4], Rc[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (double)R2w[i];
    po::quat_from_R(R, q2);
    quat_mul(p.q, q2, q);
    po::quat_to_R(q, Rc);
    const double sc = mul(p.s, 1.0);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Scw[4 * r + c] = (float)mul(sc, Rc[3 * r + c]);
        Scw[4 * r + 3] = (float)add(po::dot3(p.fwd.sR[3 * r], p.fwd.sR[3 * r + 1], p.fwd.sR[3 * r + 2], (double)t2w[0], (double)t2w[1], (double)t2w[2]), p.t[r]);
    }
    Scw[12] = Scw[13] = Scw[14] = 0.f;
    Scw[15] = 1.f;
}

FM_HD void out_zero(Out &o)
{
    for (int i = 0; i < 4; i++) o.q[i] = 0.0;
    for (int i = 0; i < 3; i++) { o.t[i] = 0.0; o.t12[i] = 0.f; }
    o.s = 0.0;
    for (int i = 0; i < 2; i++) { o.lambda[i] = o.chi2[i] = 0.0; o.iterations[i] = o.trials[i] = 0; }
    for (int i = 0; i < 9; i++) o.R12[i] = 0.f;
    for (int i = 0; i < 16; i++) o.Scw[i] = 0.f;
    o.s12 = 0.f;
    o.n_correspondences = o.n_bad_first = o.n_inliers = o.rounds = 0;
    o.status = o.skipped = o.code = 0;
}

// the head of a result: the input Sim3 (what stands when the function returns 0 ahead of the second optimisation) and the counts
FM_HD void out_begin(Out &o, const Pose &init, const float *R12, const float *t12, float s12, const float *R2w, const float *t2w, int n, int status)
{
    out_zero(o);
    for (int i = 0; i < 4; i++) o.q[i] = init.q[i];
    for (int i = 0; i < 3; i++) { o.t[i] = init.t[i]; o.t12[i] = t12[i]; }
    o.s = init.s;
    for (int i = 0; i < 9; i++) o.R12[i] = R12[i];
    o.s12 = s12;
    scw_store(init, R2w, t2w, o.Scw);
    o.n_correspondences = n;
    o.status = status;
}
FM_HD void out_round(Out &o, int round, const po::LmT<kDim, Pose> &s)
{
    o.rounds = round + 1;
    o.iterations[round] = s.iter; o.trials[round] = s.trials;
    o.lambda[round] = s.lambda; o.chi2[round] = s.currentChi;
}
// the vertex's estimate behind the second optimisation
FM_HD void out_final(Out &o, const Pose &p, const float *R2w, const float *t2w, int nInliers)
{
    double R[9];
    po::quat_to_R(p.q, R);
    for (int i = 0; i < 4; i++) o.q[i] = p.q[i];
    for (int i = 0; i < 3; i++) { o.t[i] = p.t[i]; o.t12[i] = (float)p.t[i]; }
    o.s = p.s;
    for (int i = 0; i < 9; i++) o.R12[i] = (float)R[i];
    o.s12 = (float)p.s;
    scw_store(p, R2w, t2w, o.Scw);
    o.n_inliers = nInliers;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One pair on the host, the device's order of operations with loops for its threads.  bad [n]: 1 where the correspondence was cleared (its
// row entry becomes -1).  Returns nIn.
inline int optimize_host(const Corr *corrs, int n, unsigned char *bad, const float *R12, const float *t12, float s12, float th2, int fixScale,
                         const Cams &cams, const float *R2w, const float *t2w, int status, Out &o)
{
    Pose init;
    pose_from_floats(R12, t12, s12, fixScale, init);
    out_begin(o, init, R12, t12, s12, R2w, t2w, n, status);
    for (int c = 0; c < n; c++) bad[c] = 0;
    if (n == 0) return 0;
    const double delta = huber_delta(th2);
    static thread_local po::LmT<kDim, Pose> s;
    static thread_local double part[kSums][kThreads];
    double sums[kSums];
    Pose pert[2 * kDim];
    Update upd[2 * kDim];
    for (int k = 0; k < 2 * kDim; k++) perturbation(k, fixScale, upd[k]);
    int nActive = n;
    for (int round = 0; round < 2; round++) {
        lm_round_begin(s, init, round == 0 ? kFirstIterations : (o.n_bad_first > 0 ? kMoreIterationsBad : kMoreIterationsClean));
        for (int act = po::kActIterate; act != po::kActRoundEnd;) {
            for (int k = 0; k < 2 * kDim; k++) update_apply(upd[k], s.cur, pert[k]);
            for (int t = 0; t < kThreads; t++) {
                double acc[kSums];
                for (int k = 0; k < kSums; k++) acc[k] = 0.0;
                for (int c = t; c < n; c += kThreads)
                    if (!bad[c]) corr_accumulate<1>(s.cur, pert, cams, corrs[c], delta, acc);
                for (int k = 0; k < kSums; k++) part[k][t] = acc[k];
            }
            for (int k = 0; k < kSums; k++) sums[k] = po::tree_sum(part[k]);
            lm_iteration_begin(s, sums);
            do {
                for (int t = 0; t < kThreads; t++) {
                    double acc = 0.0;
                    for (int c = t; c < n; c += kThreads)
                        if (!bad[c]) acc = corr_robust_chi2(s.trial, cams, corrs[c], delta, acc);
                    part[0][t] = acc;
                }
                act = lm_trial_done(s, po::tree_sum(part[0]));
            } while (act == po::kActTrial);
        }
        int nBad = 0;
        for (int c = 0; c < n; c++)
            if (!bad[c] && corr_is_bad(s.lastEval, cams, corrs[c], th2)) { bad[c] = 1; nBad++; }
        out_round(o, round, s);
        if (round == 0) {
            o.n_bad_first = nBad;
            nActive = n - nBad;
            if (nActive < kMinCorrespondences) return 0;
            init = s.cur;
        } else {
            out_final(o, s.cur, R2w, t2w, nActive - nBad);
        }
    }
    return o.n_inliers;
}
#endif

}  // namespace so
}  // namespace amos
