// amos_pnp_core.h -- the arithmetic of cv::solvePnPRansac(obj, img, K, 0, rvec, tvec, false, iters, err, conf, inliers, SOLVEPNP_P3P)
// (OpenCV 4.5: RANSACPointSetRegistrator with modelPoints 4 + PnPRansacCallback, p3p.cpp (Gao et al. 2003), then solvePnP(inliers,
// SOLVEPNP_EPNP), epnp.cpp (Lepetit et al. 2009)) restated from the published algorithms, written from memory of that source: PARITY WITH
// OPENCV UNPINNED.  Included by amos_pnp.hip (device), amos_flow.hip (the shared per-point error) and
// amos_reloc_pnp.hip (at the end of this file: the pieces of ORB-SLAM2's PnPsolver over the same EPnP, restated in
// tests/reloc_pnp_restatement.py; tests/host_reloc_pnp compiles them for the host; amos_sim3_core.h shares jacobi_sym, solver_iterations,
// solver_random_of and solver_draw_of with them); compilable as
// plain C++ for the host.  tests/pnp_restatement.py is the same arithmetic in Python doubles and the GPU tests hold the device to it bit
// for bit, so every value is built from + - * / sqrt only, in the written order (+ - * as written, the library builds with
// -ffp-contract=off; / and sqrt through fm::dvd / fm::sqr), every sum from 0.0 in index order.  Where OpenCV calls something else:
//   quartic of solve_for_lengths  real roots bracketed by the derivative's real roots (themselves bracketed by the cubic's critical points)
//     (solve_deg4: Ferrari)       and the Cauchy bound, then bisected until the bracket is two adjacent doubles (kBisect steps at most).
//                                 A root is a strict sign change between two bracket points, or a bracket point where the quartic is
//                                 exactly 0 (counted once).  A double root therefore counts once when the value at the critical point is
//                                 exactly 0, twice (two roots closer than ~sqrt(eps)) when rounding makes it cross, and not at all when
//                                 rounding keeps it on one side -- the same knife edge as Ferrari's D2 >= 0 / E2 >= 0 tests.
//   cvSVD of the symmetric 3 x 3  cyclic Jacobi (jacobi_sym): sweeps over (p, q) in row order, NR's negligible-element test, rotation from
//     and 12 x 12 (EPnP)          Golub & Van Loan's sym.schur2, A[p][q] set to 0; eigenvector signs fixed (largest |component| positive,
//                                 the first on ties); sorted by eigenvalue (ties: lower index first).  Negative eigenvalues of the PCA
//                                 scatter (rounding) are clamped to 0.
//   cvInvert(CC, CV_SVD)          pseudo-inverse from the Jacobi eigen-decomposition of CC^T CC, eigenvalues <= kPinvCut * largest dropped
//                                 (planar inlier sets: the third control point coincides with the centroid and its coordinate is 0)
//   cvSolve(L, rho, CV_SVD)       EPnP's own Householder qr_solve (the one its Gauss-Newton uses), x = 0 when it meets a zero column
//   cvSVD(ABt) in estimate_R_and_t  R = U V^T with v1, v2 from the Jacobi eigenvectors of ABt^T ABt, u_k = ABt v_k / |ABt v_k| and the
//                                 third pair completed by cross products (u3 = u1 x u2, v3 = v1 x v2: Kabsch, det R = +1)
//   RANSACUpdateNumIters          fm::update_num_iters with (1 - ep)^4 = q2 * q2
// Deviations kept on purpose: models are R | t (12 doubles) -- OpenCV's R -> rvec -> R Rodrigues round trip is not reproduced; the
// sampler's duplicate redraw stops after fm::kRedrawCap draws of one slot (status -2).
#pragma once

#include "amos_fmat_core.h"
#include "amos_undistort.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace amos {
namespace pnp {

using fm::dvd;
using fm::fabs_;
using fm::sqr;

constexpr int kModelPoints = 4;
constexpr int kJacobiSweeps = 50;
constexpr double kPinvCut = 1e-14;

#if defined(__HIP_DEVICE_COMPILE__)
FM_HD float fsub(float a, float b) { return __fsub_rn(a, b); }
FM_HD float fadd(float a, float b) { return __fadd_rn(a, b); }
FM_HD float fmul(float a, float b) { return __fmul_rn(a, b); }
#else
FM_HD float fsub(float a, float b) { return a - b; }
FM_HD float fadd(float a, float b) { return a + b; }
FM_HD float fmul(float a, float b) { return a * b; }
#endif

FM_HD bool finite_(double x) { return x - x == 0; }

// PnPRansacCallback::computeError for one correspondence, zero distortion: cv::projectPoints' arithmetic in doubles (X = R00 x + R01 y +
// R02 z + t0 left to right ..., 1 / Z, u = x' fx + cx stored as float), err = (float) ||img - (u, v)||^2 in float (Matx21f, NORM_L2SQR).
// M = R row-major then t.  amos_flow_pnp_score_device and k_pnp_ransac both call this.
FM_HD float point_error(const double *M, float Xf, float Yf, float Zf, float uf, float vf, double fx, double fy, double cx, double cy)
{
    const double X = Xf, Y = Yf, Z = Zf;
    const double xc = fm::add(fm::add(fm::add(fm::mul(M[0], X), fm::mul(M[1], Y)), fm::mul(M[2], Z)), M[9]);
    const double yc = fm::add(fm::add(fm::add(fm::mul(M[3], X), fm::mul(M[4], Y)), fm::mul(M[5], Z)), M[10]);
    double zc = fm::add(fm::add(fm::add(fm::mul(M[6], X), fm::mul(M[7], Y)), fm::mul(M[8], Z)), M[11]);
    zc = zc != 0.0 ? dvd(1.0, zc) : 1.0;  // cvProjectPoints2: z = z ? 1. / z : 1
    const double xn = fm::mul(xc, zc), yn = fm::mul(yc, zc);
    const float u = (float)fm::add(fm::mul(xn, fx), cx), v = (float)fm::add(fm::mul(yn, fy), cy);
    const float dx = fsub(uf, u), dy = fsub(vf, v);
    return fadd(fmul(dx, dx), fmul(dy, dy));
}

// ---- image points: solvePnPGeneric runs undistortPoints (zero distortion, P = none) on the image points, in their own depth; P3P and
// EPnP multiply the result back by fx, fy and add cx, cy in double.  P3P's sample is float (the normalised point is stored as float),
// the EPnP refit's inliers were converted to double first (the normalised point stays double).
FM_HD void pixel_p3p(float u, float v, double fx, double fy, double cx, double cy, double &pu, double &pv)
{
    const double k0[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double x, y;
    undistort_normalised(u, v, fx, fy, cx, cy, k0, x, y);
    pu = (double)(float)x * fx + cx;
    pv = (double)(float)y * fy + cy;
}

FM_HD void pixel_refit(float u, float v, double fx, double fy, double cx, double cy, double &pu, double &pv)
{
    const double k0[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double x, y;
    undistort_normalised(u, v, fx, fy, cx, cy, k0, x, y);
    pu = x * fx + cx;
    pv = y * fy + cy;
}

// ---- polynomial roots
// monic polynomial x^deg + c[0] x^(deg-1) + ... + c[deg-1] at x (Horner)
FM_HD double poly_at(const double *c, int deg, double x)
{
    double acc = x + c[0];
    for (int k = 1; k < deg; k++) acc = acc * x + c[k];
    return acc;
}

FM_HD double poly_bisect(const double *c, int deg, double lo, double hi, bool increasing)
{
    for (int it = 0; it < fm::kBisect; it++) {
        const double mid = lo * 0.5 + hi * 0.5;
        if (!(mid > lo && mid < hi)) break;
        const bool pos = poly_at(c, deg, mid) > 0;
        if (pos == increasing) hi = mid;
        else lo = mid;
    }
    return lo * 0.5 + hi * 0.5;
}

// the roots between consecutive bracket points pts[0] < ... < pts[np - 1] (at most one per interval); returns the count
FM_HD int roots_between(const double *c, int deg, const double *pts, int np, double *out)
{
    int n = 0;
    double flo = poly_at(c, deg, pts[0]);
    for (int k = 0; k + 1 < np; k++) {
        const double lo = pts[k], hi = pts[k + 1], fhi = poly_at(c, deg, hi);
        if (flo == 0) {
            if (n == 0 || out[n - 1] != lo) out[n++] = lo;
        } else if ((flo < 0 && fhi > 0) || (flo > 0 && fhi < 0)) {
            out[n++] = poly_bisect(c, deg, lo, hi, flo < 0);
        }
        flo = fhi;
    }
    return n;
}

FM_HD double clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// real roots of a x^4 + b x^3 + c x^2 + d x + e (a != 0), ascending; returns the count (0 when a coefficient is not finite)
FM_HD int solve_quartic(double a, double b, double c, double d, double e, double *r)
{
    double q[4] = {dvd(b, a), dvd(c, a), dvd(d, a), dvd(e, a)};
    if (!(finite_(q[0]) && finite_(q[1]) && finite_(q[2]) && finite_(q[3]))) return 0;
    double B4 = fabs_(q[0]);
    for (int k = 1; k < 4; k++) B4 = fabs_(q[k]) > B4 ? fabs_(q[k]) : B4;
    B4 = B4 + 1.0;
    // the derivative / 4: x^3 + 0.75 b x^2 + 0.5 c x + 0.25 d; its critical points from 3 x^2 + 2 a1 x + a2
    const double c3[3] = {0.75 * q[0], 0.5 * q[1], 0.25 * q[2]};
    double B3 = fabs_(c3[0]);
    for (int k = 1; k < 3; k++) B3 = fabs_(c3[k]) > B3 ? fabs_(c3[k]) : B3;
    B3 = B3 + 1.0;
    double p3[4];
    int np3 = 0;
    p3[np3++] = -B3;
    const double disc = c3[0] * c3[0] - 3.0 * c3[1];
    if (disc > 0) {
        const double s = sqr(disc);
        const double m1 = clampd(dvd(-c3[0] - s, 3.0), -B3, B3), m2 = clampd(dvd(-c3[0] + s, 3.0), m1, B3);
        p3[np3++] = m1;
        p3[np3++] = m2;
    }
    p3[np3++] = B3;
    double crit[3];
    const int ncrit = roots_between(c3, 3, p3, np3, crit);
    double p4[5];
    int np4 = 0;
    p4[np4++] = -B4;
    for (int k = 0; k < ncrit; k++) {
        const double prev = p4[np4 - 1];
        p4[np4++] = clampd(crit[k], prev, B4);
    }
    p4[np4++] = B4;
    return roots_between(q, 4, p4, np4, r);
}

// ---- symmetric eigen-decomposition (cyclic Jacobi); A [n][n] row-major is destroyed (its diagonal: the eigenvalues), V [n][n] receives
// the eigenvectors as columns
FM_HD void jacobi_sym(double *A, double *V, int n)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        double off = 0.0;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) off = off + fabs_(A[p * n + q]);
        if (!(off > 0)) break;  // 0, or not finite
        for (int p = 0; p + 1 < n; p++) {
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                if (apq == 0) continue;
                const double app = A[p * n + p], aqq = A[q * n + q], g = 100.0 * fabs_(apq);
                if (fabs_(app) + g == fabs_(app) && fabs_(aqq) + g == fabs_(aqq)) {
                    A[p * n + q] = 0.0;
                    A[q * n + p] = 0.0;
                    continue;
                }
                const double theta = dvd(aqq - app, 2.0 * apq);
                double t = dvd(1.0, fabs_(theta) + sqr(theta * theta + 1.0));
                if (theta < 0) t = -t;
                const double c = dvd(1.0, sqr(t * t + 1.0)), s = t * c;
                for (int k = 0; k < n; k++) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; k++) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                A[p * n + q] = 0.0;
                A[q * n + p] = 0.0;
                for (int k = 0; k < n; k++) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
        }
    }
    for (int k = 0; k < n; k++) {  // sign: the largest |component| positive (the first on ties)
        int im = 0;
        for (int i = 1; i < n; i++) im = fabs_(V[i * n + k]) > fabs_(V[im * n + k]) ? i : im;
        if (V[im * n + k] < 0)
            for (int i = 0; i < n; i++) V[i * n + k] = -V[i * n + k];
    }
}

// order[r] = index of the eigenvalue of rank r (descending when desc, else ascending; ties: lower index first)
FM_HD void eig_order(const double *A, int n, bool desc, int *order)
{
    unsigned used = 0;
    for (int r = 0; r < n; r++) {
        int best = -1;
        for (int i = 0; i < n; i++) {
            if (used & (1u << i)) continue;
            const double li = A[i * n + i];
            if (best < 0 || (desc ? li > A[best * n + best] : li < A[best * n + best])) best = i;
        }
        used |= 1u << best;
        order[r] = best;
    }
}

// ---- P3P (p3p.cpp)
FM_HD bool jacobi_4x4(double *A, double *D, double *U)
{
    double B[4], Z[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 16; i++) U[i] = (i % 5) == 0 ? 1.0 : 0.0;
    B[0] = A[0]; B[1] = A[5]; B[2] = A[10]; B[3] = A[15];
    for (int i = 0; i < 4; i++) D[i] = B[i];
    for (int iter = 0; iter < 50; iter++) {
        const double sum = fabs_(A[1]) + fabs_(A[2]) + fabs_(A[3]) + fabs_(A[6]) + fabs_(A[7]) + fabs_(A[11]);
        if (sum == 0.0) return true;
        const double tresh = iter < 3 ? dvd(0.2 * sum, 16.) : 0.0;
        for (int i = 0; i < 3; i++) {
            for (int j = i + 1; j < 4; j++) {
                double *pAij = A + 4 * i + j;
                const double Aij = *pAij, eps_machine = 100.0 * fabs_(Aij);
                if (iter > 3 && fabs_(D[i]) + eps_machine == fabs_(D[i]) && fabs_(D[j]) + eps_machine == fabs_(D[j])) {
                    *pAij = 0.0;
                } else if (fabs_(Aij) > tresh) {
                    double hh = D[j] - D[i], t;
                    if (fabs_(hh) + eps_machine == fabs_(hh)) {
                        t = dvd(Aij, hh);
                    } else {
                        const double theta = dvd(0.5 * hh, Aij);
                        t = dvd(1.0, fabs_(theta) + sqr(1.0 + theta * theta));
                        if (theta < 0.0) t = -t;
                    }
                    hh = t * Aij;
                    Z[i] -= hh; Z[j] += hh; D[i] -= hh; D[j] += hh;
                    *pAij = 0.0;
                    const double c = dvd(1.0, sqr(1 + t * t)), s = t * c, tau = dvd(s, 1.0 + c);
                    for (int k = 0; k <= i - 1; k++) {
                        const double g = A[k * 4 + i], h = A[k * 4 + j];
                        A[k * 4 + i] = g - s * (h + g * tau);
                        A[k * 4 + j] = h + s * (g - h * tau);
                    }
                    for (int k = i + 1; k <= j - 1; k++) {
                        const double g = A[i * 4 + k], h = A[k * 4 + j];
                        A[i * 4 + k] = g - s * (h + g * tau);
                        A[k * 4 + j] = h + s * (g - h * tau);
                    }
                    for (int k = j + 1; k < 4; k++) {
                        const double g = A[i * 4 + k], h = A[j * 4 + k];
                        A[i * 4 + k] = g - s * (h + g * tau);
                        A[j * 4 + k] = h + s * (g - h * tau);
                    }
                    for (int k = 0; k < 4; k++) {
                        const double g = U[k * 4 + i], h = U[k * 4 + j];
                        U[k * 4 + i] = g - s * (h + g * tau);
                        U[k * 4 + j] = h + s * (g - h * tau);
                    }
                }
            }
        }
        for (int i = 0; i < 4; i++) { B[i] += Z[i]; D[i] = B[i]; Z[i] = 0.0; }
    }
    return false;
}

// Horn's quaternion alignment of the world triangle P (P[i] = X, Y, Z of point i) onto the camera-frame points M; Rt = R row-major, t
FM_HD void align(const double M[3][3], const double P[3][3], double *Rt)
{
    double Ce[3], Cs[3], s[9];
    for (int i = 0; i < 3; i++) Ce[i] = dvd(M[0][i] + M[1][i] + M[2][i], 3);
    for (int i = 0; i < 3; i++) Cs[i] = dvd(P[0][i] + P[1][i] + P[2][i], 3);
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) s[i * 3 + j] = dvd(P[0][i] * M[0][j] + P[1][i] * M[1][j] + P[2][i] * M[2][j], 3) - Ce[j] * Cs[i];
    double Qs[16], evs[4], U[16];
    Qs[0] = s[0] + s[4] + s[8];
    Qs[5] = s[0] - s[4] - s[8];
    Qs[10] = s[4] - s[8] - s[0];
    Qs[15] = s[8] - s[0] - s[4];
    Qs[4] = Qs[1] = s[5] - s[7];
    Qs[8] = Qs[2] = s[6] - s[2];
    Qs[12] = Qs[3] = s[1] - s[3];
    Qs[9] = Qs[6] = s[3] + s[1];
    Qs[13] = Qs[7] = s[6] + s[2];
    Qs[14] = Qs[11] = s[7] + s[5];
    jacobi_4x4(Qs, evs, U);
    int iev = 0;
    double evmax = evs[0];
    for (int i = 1; i < 4; i++)
        if (evs[i] > evmax) evmax = evs[iev = i];
    double q[4];
    for (int i = 0; i < 4; i++) q[i] = U[i * 4 + iev];
    const double q02 = q[0] * q[0], q12 = q[1] * q[1], q22 = q[2] * q[2], q32 = q[3] * q[3];
    const double q0_1 = q[0] * q[1], q0_2 = q[0] * q[2], q0_3 = q[0] * q[3], q1_2 = q[1] * q[2], q1_3 = q[1] * q[3], q2_3 = q[2] * q[3];
    Rt[0] = q02 + q12 - q22 - q32;
    Rt[1] = 2. * (q1_2 - q0_3);
    Rt[2] = 2. * (q1_3 + q0_2);
    Rt[3] = 2. * (q1_2 + q0_3);
    Rt[4] = q02 + q22 - q12 - q32;
    Rt[5] = 2. * (q2_3 - q0_1);
    Rt[6] = 2. * (q1_3 - q0_2);
    Rt[7] = 2. * (q2_3 + q0_1);
    Rt[8] = q02 + q32 - q12 - q22;
    for (int i = 0; i < 3; i++) Rt[9 + i] = Ce[i] - (Rt[3 * i] * Cs[0] + Rt[3 * i + 1] * Cs[1] + Rt[3 * i + 2] * Cs[2]);
}

FM_HD int solve_for_lengths(double lengths[4][3], const double *distances, const double *cosines)
{
    const double p = cosines[0] * 2, q = cosines[1] * 2, r = cosines[2] * 2;
    const double inv_d22 = dvd(1., distances[2] * distances[2]);
    const double a = inv_d22 * (distances[0] * distances[0]), b = inv_d22 * (distances[1] * distances[1]);
    const double a2 = a * a, b2 = b * b, p2 = p * p, q2 = q * q, r2 = r * r, pr = p * r, pqr = q * pr;
    if (p2 + q2 + r2 - pqr - 1 == 0) return 0;
    const double ab = a * b, a_2 = 2 * a;
    const double A = -2 * b + b2 + a2 + 1 + ab * (2 - r2) - a_2;
    if (A == 0) return 0;
    const double a_4 = 4 * a;
    const double B = q * (-2 * (ab + a2 + 1 - b) + r2 * ab + a_4) + pr * (b - b2 + ab);
    const double C = q2 + b2 * (r2 + p2 - 2) - b * (p2 + pqr) - ab * (r2 + pqr) + (a2 - a_2) * (2 + q2) + 2;
    const double D = pr * (ab - b2 + b) + q * ((p2 - 2) * b + 2 * (ab - a2) + a_4 - 2);
    const double E = 1 + 2 * (b - a - ab) + b2 - b * p2 + a2;
    const double temp = p2 * (a - 1 + b) + r2 * (a - 1 - b) + pqr - a * pqr;
    const double b0 = b * temp * temp;
    if (b0 == 0) return 0;
    double real_roots[4];
    const int n = solve_quartic(A, B, C, D, E, real_roots);
    if (n == 0) return 0;
    int nb = 0;
    const double r3 = r2 * r, pr2 = p * r2, r3q = r3 * q, inv_b0 = dvd(1., b0);
    for (int i = 0; i < n; i++) {
        const double x = real_roots[i];
        if (x <= 0) continue;
        const double x2 = x * x;
        const double b1 =
            ((1 - a - b) * x2 + (q * a - q) * x + 1 - a + b) *
            (((r3 * (a2 + ab * (2 - r2) - a_2 + b2 - 2 * b + 1)) * x +
              (r3q * (2 * (b - a2) + a_4 + ab * (r2 - 2) - 2) + pr2 * (1 + a2 + 2 * (ab - a - b) + r2 * (b - b2) + b2))) * x2 +
             (r3 * (q2 * (1 - 2 * a + a2) + r2 * (b2 - ab) - a_4 + 2 * (a2 - b2) + 2) + r * p2 * (b2 + 2 * (ab - b - a) + 1 + a2) +
              pr2 * q * (a_4 + 2 * (b - ab - a2) - 2 - r2 * b)) * x +
             2 * r3q * (a_2 - b - a2 + ab - 1) + pr2 * (q2 - a_4 + 2 * (a2 - b2) + r2 * b + q2 * (a2 - a_2) + 2) +
             p2 * (p * (2 * (ab - a - b) + a2 + b2 + 1) + 2 * q * r * (b + a_2 - a2 - ab - 1)));
        if (b1 <= 0) continue;
        const double y = inv_b0 * b1, v = x2 + y * y - x * y * r;
        if (v <= 0) continue;
        const double Z = dvd(distances[2], sqr(v));
        lengths[nb][0] = x * Z;
        lengths[nb][1] = y * Z;
        lengths[nb][2] = Z;
        nb++;
    }
    return nb;
}

// p3p::solve on four correspondences (obj: x, y, z floats; img: pixel floats): the solutions of the first three, the one with the smallest
// squared reprojection error of the fourth (the first on ties).  Returns false for no model, including any non-finite R | t.
FM_HD bool p3p4(const float *obj, const float *img, double fx, double fy, double cx, double cy, double *Rt)
{
    double mu[4], mv[4];
    for (int i = 0; i < 4; i++) pixel_p3p(img[2 * i], img[2 * i + 1], fx, fy, cx, cy, mu[i], mv[i]);
    const double inv_fx = dvd(1., fx), inv_fy = dvd(1., fy), cx_fx = dvd(cx, fx), cy_fy = dvd(cy, fy);
    double P[3][3], u[3], v[3], k[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) P[i][j] = obj[3 * i + j];
        u[i] = inv_fx * mu[i] - cx_fx;
        v[i] = inv_fy * mv[i] - cy_fy;
        const double norm = sqr(u[i] * u[i] + v[i] * v[i] + 1);
        k[i] = dvd(1., norm);
        u[i] *= k[i];
        v[i] *= k[i];
    }
    auto d2 = [&](int i, int j) {
        return (P[i][0] - P[j][0]) * (P[i][0] - P[j][0]) + (P[i][1] - P[j][1]) * (P[i][1] - P[j][1]) + (P[i][2] - P[j][2]) * (P[i][2] - P[j][2]);
    };
    const double distances[3] = {sqr(d2(1, 2)), sqr(d2(0, 2)), sqr(d2(0, 1))};
    const double cosines[3] = {u[1] * u[2] + v[1] * v[2] + k[1] * k[2], u[0] * u[2] + v[0] * v[2] + k[0] * k[2], u[0] * u[1] + v[0] * v[1] + k[0] * k[1]};
    double lengths[4][3];
    const int n = solve_for_lengths(lengths, distances, cosines);
    if (n == 0) return false;
    const double X3 = obj[9], Y3 = obj[10], Z3 = obj[11];
    double best = 0.0;
    bool found = false;
    for (int s = 0; s < n; s++) {
        double M[3][3], cand[12];
        for (int i = 0; i < 3; i++) {
            M[i][0] = lengths[s][i] * u[i];
            M[i][1] = lengths[s][i] * v[i];
            M[i][2] = lengths[s][i] * k[i];
        }
        align(M, P, cand);
        const double X3p = cand[0] * X3 + cand[1] * Y3 + cand[2] * Z3 + cand[9];
        const double Y3p = cand[3] * X3 + cand[4] * Y3 + cand[5] * Z3 + cand[10];
        const double Z3p = cand[6] * X3 + cand[7] * Y3 + cand[8] * Z3 + cand[11];
        const double mu3p = cx + dvd(fx * X3p, Z3p), mv3p = cy + dvd(fy * Y3p, Z3p);
        const double reproj = (mu3p - mu[3]) * (mu3p - mu[3]) + (mv3p - mv[3]) * (mv3p - mv[3]);
        if (s == 0 || best > reproj) {
            best = reproj;
            for (int i = 0; i < 12; i++) Rt[i] = cand[i];
            found = true;
        }
    }
    bool ok = found;
    for (int i = 0; i < 12; i++) ok = ok && finite_(Rt[i]);
    return ok;
}

// RANSACUpdateNumIters(p, ep, 4, maxIters)
FM_HD int update_num_iters(double p, double ep, int maxIters) { return fm::update_num_iters(p, ep, maxIters, kModelPoints); }

// ---- EPnP (epnp.cpp) building blocks; the per-point ones are called in index order by whichever lane owns the sum
// alphas of one point: ci = pinv(CC) row-major, cw0 = control point 0
FM_HD void alphas(const double *ci, const double *cw0, double X, double Y, double Z, double *a)
{
    for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * (X - cw0[0]) + ci[3 * j + 1] * (Y - cw0[1]) + ci[3 * j + 2] * (Z - cw0[2]);
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

// entry c (0..11) of the two rows of M for one point (fill_M)
FM_HD void m_entries(const double *a, double u, double v, double fu, double fv, double uc, double vc, int c, double &m1, double &m2)
{
    const double as = a[c / 3];
    const int comp = c % 3;
    m1 = comp == 0 ? as * fu : (comp == 1 ? 0.0 : as * (uc - u));
    m2 = comp == 0 ? 0.0 : (comp == 1 ? as * fv : as * (vc - v));
}

FM_HD double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
FM_HD double dist2(const double *a, const double *b)
{
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// control points 1..3 from the PCA scatter S [3][3] of the inliers about cw[0]; ci = pinv(CC).  S is destroyed.
FM_HD void control_points(double *S, int m, double cw[4][3], double *ci)
{
    double V[9], G[9], W[9], CC[9];
    int order[3];
    jacobi_sym(S, V, 3);
    eig_order(S, 3, true, order);
    for (int i = 1; i < 4; i++) {
        double dc = S[order[i - 1] * 4];
        dc = dc < 0 ? 0.0 : dc;
        const double kk = sqr(dvd(dc, (double)m));
        for (int j = 0; j < 3; j++) cw[i][j] = cw[0][j] + kk * V[j * 3 + order[i - 1]];
    }
    for (int i = 0; i < 3; i++)
        for (int j = 1; j < 4; j++) CC[3 * i + j - 1] = cw[j][i] - cw[0][i];
    // pinv(CC) = V diag(1 / l) V^T CC^T with CC^T CC = V diag(l) V^T, l <= kPinvCut * max dropped
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            double acc = 0.0;
            for (int r = 0; r < 3; r++) acc = acc + CC[3 * r + a] * CC[3 * r + b];
            G[3 * a + b] = acc;
        }
    jacobi_sym(G, V, 3);
    double lmax = G[0], inv[3];
    lmax = G[4] > lmax ? G[4] : lmax;
    lmax = G[8] > lmax ? G[8] : lmax;
    for (int k = 0; k < 3; k++) inv[k] = G[4 * k] > kPinvCut * lmax ? dvd(1.0, G[4 * k]) : 0.0;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            double acc = 0.0;
            for (int k = 0; k < 3; k++) acc = acc + V[3 * a + k] * inv[k] * V[3 * b + k];
            W[3 * a + b] = acc;
        }
    for (int a = 0; a < 3; a++)
        for (int r = 0; r < 3; r++) {
            double acc = 0.0;
            for (int b = 0; b < 3; b++) acc = acc + W[3 * a + b] * CC[3 * r + b];
            ci[3 * a + r] = acc;
        }
}

// EPnP's qr_solve (Householder, its own pivot-free form) on A [nr][nc] (destroyed), b [nr] (destroyed); x untouched when a column is 0
FM_HD void qr_solve(double *A, int nr, int nc, double *b, double *x)
{
    double A1[6], A2[6];
    for (int k = 0; k < nc; k++) {
        double eta = fabs_(A[k * nc + k]);
        for (int i = k + 1; i < nr; i++) eta = eta < fabs_(A[i * nc + k]) ? fabs_(A[i * nc + k]) : eta;
        if (eta == 0) return;
        double sum2 = 0.0;
        const double inv_eta = dvd(1., eta);
        for (int i = k; i < nr; i++) {
            A[i * nc + k] *= inv_eta;
            sum2 += A[i * nc + k] * A[i * nc + k];
        }
        double sigma = sqr(sum2);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] += sigma;
        A1[k] = sigma * A[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double sum = 0;
            for (int i = k; i < nr; i++) sum += A[i * nc + k] * A[i * nc + j];
            const double tau = dvd(sum, A1[k]);
            for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {
        double tau = 0;
        for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
        tau = dvd(tau, A1[j]);
        for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
    }
    x[nc - 1] = dvd(b[nc - 1], A2[nc - 1]);
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
        for (int j = i + 1; j < nc; j++) sum += A[i * nc + j] * x[j];
        x[i] = dvd(b[i] - sum, A2[i]);
    }
}

// L_6x10 from the four null-space vectors v[i] (v[0]: smallest eigenvalue), rho from the control points
FM_HD void l6x10_rho(const double v[4][12], const double cw[4][3], double *L, double *rho)
{
    double dv[4][6][3];
    for (int i = 0; i < 4; i++) {
        int a = 0, b = 1;
        for (int j = 0; j < 6; j++) {
            for (int k = 0; k < 3; k++) dv[i][j][k] = v[i][3 * a + k] - v[i][3 * b + k];
            b++;
            if (b > 3) { a++; b = a + 1; }
        }
    }
    for (int i = 0; i < 6; i++) {
        double *row = L + 10 * i;
        row[0] = dot3(dv[0][i], dv[0][i]);
        row[1] = 2.0 * dot3(dv[0][i], dv[1][i]);
        row[2] = dot3(dv[1][i], dv[1][i]);
        row[3] = 2.0 * dot3(dv[0][i], dv[2][i]);
        row[4] = 2.0 * dot3(dv[1][i], dv[2][i]);
        row[5] = dot3(dv[2][i], dv[2][i]);
        row[6] = 2.0 * dot3(dv[0][i], dv[3][i]);
        row[7] = 2.0 * dot3(dv[1][i], dv[3][i]);
        row[8] = 2.0 * dot3(dv[2][i], dv[3][i]);
        row[9] = dot3(dv[3][i], dv[3][i]);
    }
    rho[0] = dist2(cw[0], cw[1]); rho[1] = dist2(cw[0], cw[2]); rho[2] = dist2(cw[0], cw[3]);
    rho[3] = dist2(cw[1], cw[2]); rho[4] = dist2(cw[1], cw[3]); rho[5] = dist2(cw[2], cw[3]);
}

// find_betas_approx_{1,2,3} (which = 1, 2, 3), then gauss_newton's 5 steps
FM_HD void betas_for(const double *L, const double *rho, int which, double *betas)
{
    const int nc = which == 1 ? 4 : (which == 2 ? 3 : 5);
    double A[30], b[6], x[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j < nc; j++) A[i * nc + j] = L[10 * i + (which == 1 && j >= 2 ? 3 * j - 3 : j)];  // approx 1: columns 0, 1, 3, 6
        b[i] = rho[i];
    }
    qr_solve(A, 6, nc, b, x);
    if (which == 1) {
        if (x[0] < 0) {
            betas[0] = sqr(-x[0]);
            betas[1] = dvd(-x[1], betas[0]); betas[2] = dvd(-x[2], betas[0]); betas[3] = dvd(-x[3], betas[0]);
        } else {
            betas[0] = sqr(x[0]);
            betas[1] = dvd(x[1], betas[0]); betas[2] = dvd(x[2], betas[0]); betas[3] = dvd(x[3], betas[0]);
        }
    } else {
        if (x[0] < 0) {
            betas[0] = sqr(-x[0]);
            betas[1] = x[2] < 0 ? sqr(-x[2]) : 0.0;
        } else {
            betas[0] = sqr(x[0]);
            betas[1] = x[2] > 0 ? sqr(x[2]) : 0.0;
        }
        if (x[1] < 0) betas[0] = -betas[0];
        betas[2] = which == 3 ? dvd(x[3], betas[0]) : 0.0;
        betas[3] = 0.0;
    }
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it < 5; it++) {
        double GA[24], gb[6];
        for (int i = 0; i < 6; i++) {
            const double *l = L + 10 * i;
            GA[4 * i + 0] = 2 * l[0] * betas[0] + l[1] * betas[1] + l[3] * betas[2] + l[6] * betas[3];
            GA[4 * i + 1] = l[1] * betas[0] + 2 * l[2] * betas[1] + l[4] * betas[2] + l[7] * betas[3];
            GA[4 * i + 2] = l[3] * betas[0] + l[4] * betas[1] + 2 * l[5] * betas[2] + l[8] * betas[3];
            GA[4 * i + 3] = l[6] * betas[0] + l[7] * betas[1] + l[8] * betas[2] + 2 * l[9] * betas[3];
            gb[i] = rho[i] - (l[0] * betas[0] * betas[0] + l[1] * betas[0] * betas[1] + l[2] * betas[1] * betas[1] + l[3] * betas[0] * betas[2] +
                              l[4] * betas[1] * betas[2] + l[5] * betas[2] * betas[2] + l[6] * betas[0] * betas[3] + l[7] * betas[1] * betas[3] +
                              l[8] * betas[2] * betas[3] + l[9] * betas[3] * betas[3]);
        }
        qr_solve(GA, 6, 4, gb, g);
        for (int i = 0; i < 4; i++) betas[i] += g[i];
    }
}

// compute_ccs: the camera-frame control points from betas and the null-space vectors
FM_HD void ccs_of(const double *betas, const double v[4][12], double ccs[4][3])
{
    for (int j = 0; j < 4; j++)
        for (int k = 0; k < 3; k++) ccs[j][k] = 0.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * v[i][3 * j + k];
}

FM_HD void pc_of(const double *a, const double ccs[4][3], bool neg, double *pc)
{
    for (int j = 0; j < 3; j++) {
        const double x = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
        pc[j] = neg ? -x : x;
    }
}

// estimate_R_and_t from the sums: H = ABt [3][3] (abt[3 j + k] = sum (pc_j - pc0_j)(pw_k - pw0_k)), pc0, pw0 the means
FM_HD void r_and_t(const double *H, const double *pc0, const double *pw0, double *Rt)
{
    double G[9], V[9];
    int order[3];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            double acc = 0.0;
            for (int r = 0; r < 3; r++) acc = acc + H[3 * r + a] * H[3 * r + b];
            G[3 * a + b] = acc;
        }
    jacobi_sym(G, V, 3);
    eig_order(G, 3, true, order);
    double vv[3][3], uu[3][3];
    for (int k = 0; k < 2; k++) {
        for (int i = 0; i < 3; i++) vv[k][i] = V[3 * i + order[k]];
        double hv[3];
        for (int i = 0; i < 3; i++) hv[i] = H[3 * i] * vv[k][0] + H[3 * i + 1] * vv[k][1] + H[3 * i + 2] * vv[k][2];
        const double nn = sqr(dot3(hv, hv));
        for (int i = 0; i < 3; i++) uu[k][i] = dvd(hv[i], nn);
    }
    vv[2][0] = vv[0][1] * vv[1][2] - vv[0][2] * vv[1][1];
    vv[2][1] = vv[0][2] * vv[1][0] - vv[0][0] * vv[1][2];
    vv[2][2] = vv[0][0] * vv[1][1] - vv[0][1] * vv[1][0];
    uu[2][0] = uu[0][1] * uu[1][2] - uu[0][2] * uu[1][1];
    uu[2][1] = uu[0][2] * uu[1][0] - uu[0][0] * uu[1][2];
    uu[2][2] = uu[0][0] * uu[1][1] - uu[0][1] * uu[1][0];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rt[3 * i + j] = uu[0][i] * vv[0][j] + uu[1][i] * vv[1][j] + uu[2][i] * vv[2][j];
    const double det = Rt[0] * Rt[4] * Rt[8] + Rt[1] * Rt[5] * Rt[6] + Rt[2] * Rt[3] * Rt[7] - Rt[2] * Rt[4] * Rt[6] - Rt[1] * Rt[3] * Rt[8] -
                       Rt[0] * Rt[5] * Rt[7];
    if (det < 0) { Rt[6] = -Rt[6]; Rt[7] = -Rt[7]; Rt[8] = -Rt[8]; }
    for (int i = 0; i < 3; i++) Rt[9 + i] = pc0[i] - dot3(Rt + 3 * i, pw0);
}

// one term of reprojection_error: sqrt of the squared pixel distance of one point under Rt
FM_HD double reproj_term(const double *Rt, const double *pw, double u, double v, double fu, double fv, double uc, double vc)
{
    const double Xc = dot3(Rt, pw) + Rt[9], Yc = dot3(Rt + 3, pw) + Rt[10];
    const double inv_Zc = dvd(1.0, dot3(Rt + 6, pw) + Rt[11]);
    const double ue = uc + fu * Xc * inv_Zc, ve = vc + fv * Yc * inv_Zc;
    return sqr((u - ue) * (u - ue) + (v - ve) * (v - ve));
}

// ---- the image point an EPnP reads, as a policy: solvePnP's refit sends the pixel through undistortPoints and back (pixel_refit),
// ORB-SLAM2's PnPsolver hands EPnP the pixel as it is
struct PixelRefit {
    static FM_HD void at(float u, float v, double fx, double fy, double cx, double cy, double &pu, double &pv) { pixel_refit(u, v, fx, fy, cx, cy, pu, pv); }
};
struct PixelDirect {
    static FM_HD void at(float u, float v, double, double, double, double, double &pu, double &pv) { pu = (double)u; pv = (double)v; }
};

constexpr int kEpnpScratch = 6;  // doubles per point: alphas[4], u, v

// EPnP on m >= 4 points on ONE thread: the steps and the summation order of the block-wide form (amos_pnp_block.h), every sum from 0.0 in
// point order.  point_of(j, pw, u, v) gives point j (world doubles, pixel floats); scr holds kEpnpScratch * m doubles; MtM and E hold 144
// doubles each (in LDS on the device).  Rt is the beta set with the smallest mean reprojection error, not tested for finiteness.
// jacobi12(MtM, E) is the 12 x 12 eigen-decomposition: jacobi_sym on one thread (Jacobi12Serial), or a form that applies the same rotations
// with several lanes (amos_pnp_block.h: the lanes of a group then call epnp_serial together, on the same points and the same MtM / E).
struct Jacobi12Serial {
    FM_HD void operator()(double *A, double *V) const { jacobi_sym(A, V, 12); }
};

template <class Pixel, class PointOf, class Jacobi12 = Jacobi12Serial>
FM_HD void epnp_serial(int m, PointOf point_of, double fx, double fy, double cx, double cy, double *scr, double *MtM, double *E, double *Rt,
                       Jacobi12 jacobi12 = Jacobi12())
{
    const double dm = (double)m;
    double cw[4][3], S[9], ci[9], pw[3];
    float uf, vf;
    for (int c = 0; c < 3; c++) {
        double acc = 0.0;
        for (int j = 0; j < m; j++) { point_of(j, pw, uf, vf); acc = acc + pw[c]; }
        cw[0][c] = dvd(acc, dm);
    }
    for (int r = 0; r < 3; r++)
        for (int c = r; c < 3; c++) {
            double acc = 0.0;
            for (int j = 0; j < m; j++) { point_of(j, pw, uf, vf); acc = acc + (pw[r] - cw[0][r]) * (pw[c] - cw[0][c]); }
            S[3 * r + c] = acc;
            S[3 * c + r] = acc;
        }
    control_points(S, m, cw, ci);
    for (int j = 0; j < m; j++) {
        double *o = scr + (size_t)j * kEpnpScratch;
        point_of(j, pw, uf, vf);
        alphas(ci, cw[0], pw[0], pw[1], pw[2], o);
        Pixel::at(uf, vf, fx, fy, cx, cy, o[4], o[5]);
    }
    for (int r = 0; r < 12; r++)
        for (int c = r; c < 12; c++) {
            double acc = 0.0;
            for (int j = 0; j < m; j++) {
                const double *o = scr + (size_t)j * kEpnpScratch;
                double r1, r2, c1, c2;
                m_entries(o, o[4], o[5], fx, fy, cx, cy, r, r1, r2);
                m_entries(o, o[4], o[5], fx, fy, cx, cy, c, c1, c2);
                acc = acc + r1 * c1;
                acc = acc + r2 * c2;
            }
            MtM[12 * r + c] = acc;
            MtM[12 * c + r] = acc;
        }
    jacobi12(MtM, E);
    int order[12];
    eig_order(MtM, 12, false, order);
    double v[4][12], L[60], rho[6];
    for (int i = 0; i < 4; i++)
        for (int k = 0; k < 12; k++) v[i][k] = E[12 * k + order[i]];
    l6x10_rho(v, cw, L, rho);
    double bestRep = 0.0;
    for (int w = 0; w < 3; w++) {
        double betas[4], ccs[4][3], pc[3], sum[6], H[9], cand[12];
        betas_for(L, rho, w + 1, betas);
        ccs_of(betas, v, ccs);
        pc_of(scr, ccs, false, pc);  // the first point decides solve_for_sign
        const bool neg = pc[2] < 0.0;
        for (int q = 0; q < 6; q++) {
            double acc = 0.0;
            for (int j = 0; j < m; j++) {
                double x;
                if (q < 3) { pc_of(scr + (size_t)j * kEpnpScratch, ccs, neg, pc); x = pc[q]; }
                else { point_of(j, pw, uf, vf); x = pw[q - 3]; }
                acc = acc + x;
            }
            sum[q] = dvd(acc, dm);
        }
        for (int e = 0; e < 9; e++) {
            const int r = e / 3, c = e % 3;
            double acc = 0.0;
            for (int j = 0; j < m; j++) {
                pc_of(scr + (size_t)j * kEpnpScratch, ccs, neg, pc);
                point_of(j, pw, uf, vf);
                acc = acc + (pc[r] - sum[r]) * (pw[c] - sum[3 + c]);
            }
            H[e] = acc;
        }
        r_and_t(H, sum, sum + 3, cand);
        double acc = 0.0;
        for (int j = 0; j < m; j++) {
            const double *o = scr + (size_t)j * kEpnpScratch;
            point_of(j, pw, uf, vf);
            acc = acc + reproj_term(cand, pw, o[4], o[5], fx, fy, cx, cy);
        }
        const double rep = dvd(acc, dm);
        if (w == 0 || rep < bestRep) {
            bestRep = rep;
            for (int k = 0; k < 12; k++) Rt[k] = cand[k];
        }
    }
}

// ---- ORB-SLAM2's PnPsolver (src/PnPsolver.cc:120-458), the per-iteration pieces; tests/reloc_pnp_restatement.py is the same in Python
constexpr int kSolverMaxPoints = 4096;

// the iteration count of a SetRansacParameters: ceil(log(1 - p) / log(1 - eps^3)) (PnPsolver.cc:213, Sim3Solver.cc:182).  log is fm::log_,
// pow(eps, 3) = (e e) e.  Where the reference converts a NaN or a huge double to int: 1 - e^3 <= 0 gives one iteration, a log that is not
// negative or a quotient >= maxIterations gives maxIterations.
FM_HD int solver_iterations(float eps, double probability, int maxIterations)
{
    const double e = (double)eps, arg = fm::sub(1.0, fm::mul(fm::mul(e, e), e));
    if (!(arg > 0)) return 1;
    const double num = fm::log_(fm::sub(1.0, probability)), den = fm::log_(arg);
    if (!(den < 0)) return maxIterations;
    const double quot = dvd(num, den);
    return quot >= (double)maxIterations ? maxIterations : (int)ceil(quot);
}

// SetRansacParameters(probability, minInliers, maxIterations, 4, epsilon, .) for N correspondences: the adjusted minInliers, maxIts and
// epsilon.
FM_HD void solver_parameters(int N, double probability, int minInliers, int maxIterations, float epsilon, int &nMin, int &maxIts, float &eps)
{
    eps = epsilon;
    const float scaled = fmul((float)N, eps);
    nMin = scaled < 1073741824.f ? (int)scaled : 1073741824;  // (the reference's conversion of a larger float is undefined)
    if (nMin < minInliers) nMin = minInliers;
    if (nMin < 4) nMin = 4;
    if (N > 0) {
#if defined(__HIP_DEVICE_COMPILE__)
        const float q = __fdiv_rn((float)nMin, (float)N);
#else
        const float q = (float)nMin / (float)N;
#endif
        if (eps < q) eps = q;
    }
    int nIt = nMin == N ? 1 : solver_iterations(eps, probability, maxIterations);
    nIt = nIt < maxIterations ? nIt : maxIterations;
    maxIts = nIt > 1 ? nIt : 1;
}

// DUtils::Random::RandomInt(0, s - 1) with a 31-bit rand() drawn from the solver's generator (r: its next 32 bits)
FM_HD int solver_random_of(uint32_t r, int s) { return (int)fm::mul(dvd((double)(r >> 1), 2147483648.0), (double)s); }
FM_HD int solver_random_int(uint64_t &rng, int s) { return solver_random_of(fm::rng_next(rng), s); }

// the K draws of one iteration (PnPsolver.cc:268-283 with four, Sim3Solver.cc:228-249 with three) without the copied index list: the
// swap-with-back of slot k is one entry of a substitution table (position -> the entry moved there), the latest entry of a position wins.
// next() hands out the generator's 32-bit outputs in order (drawn ahead by one lane, or straight from the state)
template <int K, class Next>
FM_HD void solver_draw_of(Next next, int N, int *idx)
{
    int pos[K], val[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int s = N - k, randi = solver_random_of(next(), s);
        int a = randi, b = s - 1;
        bool fa = false, fb = false;
#pragma unroll
        for (int q = k - 1; q >= 0; q--) {
            if (!fa && pos[q] == randi) { a = val[q]; fa = true; }
            if (!fb && pos[q] == s - 1) { b = val[q]; fb = true; }
        }
        idx[k] = a;
        pos[k] = randi;
        val[k] = b;
    }
}
template <int K>
FM_HD void solver_draw(uint64_t &rng, int N, int *idx)
{
    solver_draw_of<K>([&rng]() { return fm::rng_next(rng); }, N, idx);
}
FM_HD void solver_draw4(uint64_t &rng, int N, int *idx) { solver_draw<4>(rng, N, idx); }

// CheckInliers for one correspondence: every operation rounded, the float stores of the reference kept
FM_HD bool solver_inlier(const double *Rt, float Xf, float Yf, float Zf, float uf, float vf, double fu, double fv, double uc, double vc, float maxErr)
{
    const double X = Xf, Y = Yf, Z = Zf;
    const float Xc = (float)fm::add(fm::add(fm::add(fm::mul(Rt[0], X), fm::mul(Rt[1], Y)), fm::mul(Rt[2], Z)), Rt[9]);
    const float Yc = (float)fm::add(fm::add(fm::add(fm::mul(Rt[3], X), fm::mul(Rt[4], Y)), fm::mul(Rt[5], Z)), Rt[10]);
    const float invZc = (float)dvd(1.0, fm::add(fm::add(fm::add(fm::mul(Rt[6], X), fm::mul(Rt[7], Y)), fm::mul(Rt[8], Z)), Rt[11]));
    const double ue = fm::add(uc, fm::mul(fm::mul(fu, (double)Xc), (double)invZc));
    const double ve = fm::add(vc, fm::mul(fm::mul(fv, (double)Yc), (double)invZc));
    const float distX = (float)fm::sub((double)uf, ue), distY = (float)fm::sub((double)vf, ve);
    const float error2 = fadd(fmul(distX, distX), fmul(distY, distY));
    return error2 < maxErr;
}

// rows of [R | t] as float: what the reference's convertTo(CV_32F) and copyTo into mBestTcw / mRefinedTcw store
FM_HD void solver_tcw(const double *Rt, float *Tcw)
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Tcw[4 * r + c] = (float)Rt[3 * r + c];
        Tcw[4 * r + 3] = (float)Rt[9 + r];
    }
}

}  // namespace pnp
}  // namespace amos
