// amos_fmat_core.h -- the arithmetic of cv::findFundamentalMat(p1, p2, FM_RANSAC, threshold, confidence) (OpenCV 4.5's classic
// RANSACPointSetRegistrator + FMEstimatorCallback, modules/calib3d/src/{fundam,ptsetreg}.cpp) restated from the published
// algorithm, written from memory of that source: PARITY WITH OPENCV UNPINNED.  Included by amos_fmat.hip (device)
// and compilable as plain C++ for the host; tests/fmat_restatement.py is the same arithmetic in Python doubles and the GPU tests hold
// the device to it bit for bit.  So every value is built from + - * / sqrt only (correctly rounded on both sides, no fused
// multiply-add: the library builds with -ffp-contract=off), in a fixed order; where OpenCV calls an SVD, acos / cos / pow (cubic) or
// log / pow (iteration count) the restatement uses:
//   null space of the 7 x 9 system   Householder QR of its transpose (7 reflections, fixed order); the last two columns of Q
//   cubic det(l f1 + f2) = 0         cv::solveCubic's branches and root count (d > 0 and Q > 0: three roots); each real root bracketed
//                                    by the critical points and the Cauchy bound, then bisected until the bracket is two adjacent
//                                    doubles (at most kBisect steps)
//   RANSACUpdateNumIters             log from frexp + a 12-term atanh series; (1 - ep)^7 as a fixed multiplication chain
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FM_HD __host__ __device__ __forceinline__
#else
#define FM_HD inline
#endif

namespace amos {
namespace fm {

constexpr int kModelPoints = 7;
constexpr int kMaxAttempts = 10000;        // getSubset(..., 10000) in RANSACPointSetRegistrator::run
constexpr uint32_t kRedrawCap = 1u << 20;  // draws of one subset slot (OpenCV's duplicate redraw is unbounded; documented cap)
constexpr int kBisect = 160;
constexpr double kDblEpsilon = 2.220446049250313e-16;
constexpr double kDblMin = 2.2250738585072014e-308;
constexpr double kFltEpsilon = 1.1920928955078125e-07;
constexpr double kLn2 = 0.6931471805599453;
constexpr double kSqrtHalf = 0.7071067811865476;

#if defined(__HIP_DEVICE_COMPILE__)
FM_HD double add(double a, double b) { return __dadd_rn(a, b); }
FM_HD double sub(double a, double b) { return __dsub_rn(a, b); }
FM_HD double mul(double a, double b) { return __dmul_rn(a, b); }
FM_HD double dvd(double a, double b) { return __ddiv_rn(a, b); }
FM_HD double sqr(double a) { return __dsqrt_rn(a); }
#else
FM_HD double add(double a, double b) { return a + b; }
FM_HD double sub(double a, double b) { return a - b; }
FM_HD double mul(double a, double b) { return a * b; }
FM_HD double dvd(double a, double b) { return a / b; }
FM_HD double sqr(double a) { return std::sqrt(a); }
#endif
FM_HD double fabs_(double a) { return a < 0 ? -a : a; }

// cv::RNG: state = (uint64)(uint32)state * 4164903690 + (state >> 32); next() = low 32 bits; uniform(0, n) = next() % n
FM_HD uint32_t rng_next(uint64_t &s)
{
    s = (uint64_t)(uint32_t)s * 4164903690u + (s >> 32);
    return (uint32_t)s;
}

// one test of haveCollinearPoints(m, 7): the last selected point i against the pair (j, k), k < j < i.  Differences are float
// subtractions (Point2f - Point2f), the test in doubles.
FM_HD bool collinear3(float xj, float yj, float xk, float yk, float xi, float yi)
{
    const double dx1 = (double)(xj - xi), dy1 = (double)(yj - yi);
    const double dx2 = (double)(xk - xi), dy2 = (double)(yk - yi);
    const double lhs = fabs_(sub(mul(dx2, dy1), mul(dy2, dx1)));
    const double rhs = mul(kFltEpsilon, add(add(add(fabs_(dx1), fabs_(dy1)), fabs_(dx2)), fabs_(dy2)));
    return lhs <= rhs;
}

// the 15 pairs (j, k), k < j < 6, in OpenCV's loop order: pair p -> (FM_PAIR_J(p), FM_PAIR_K(p))
#define FM_PAIR_J(p) ((p) < 1 ? 1 : (p) < 3 ? 2 : (p) < 6 ? 3 : (p) < 10 ? 4 : 5)
#define FM_PAIR_K(p) ((p) - (FM_PAIR_J(p) * (FM_PAIR_J(p) - 1)) / 2)

// the monic cubic x^3 + a1 x^2 + a2 x + a3 at x (Horner)
FM_HD double cubic_at(double a1, double a2, double a3, double x) { return add(mul(add(mul(add(x, a1), x), a2), x), a3); }

// bisection of [lo, hi] towards the sign change (increasing: p(lo) <= 0 < p(hi)), until the bracket cannot shrink
FM_HD double bisect(double a1, double a2, double a3, double lo, double hi, bool increasing)
{
    for (int it = 0; it < kBisect; it++) {
        const double mid = add(mul(lo, 0.5), mul(hi, 0.5));
        if (!(mid > lo && mid < hi)) break;
        const bool pos = cubic_at(a1, a2, a3, mid) > 0;
        if (pos == increasing) hi = mid;
        else lo = mid;
    }
    return add(mul(lo, 0.5), mul(hi, 0.5));
}

// cv::solveCubic's case split for c[0] x^3 + c[1] x^2 + c[2] x + c[3]; returns the root count (-1: every x is a root)
FM_HD int solve_cubic(const double *c, double *r)
{
    double a0 = c[0], a1 = c[1], a2 = c[2], a3 = c[3];
    if (a0 == 0) {
        if (a1 == 0) {
            if (a2 == 0) return a3 == 0 ? -1 : 0;
            r[0] = dvd(-a3, a2);
            return 1;
        }
        double d = sub(mul(a2, a2), mul(mul(4.0, a1), a3));
        if (!(d >= 0)) return 0;
        d = sqr(d);
        const double q1 = mul(add(-a2, d), 0.5), q2 = mul(add(a2, d), -0.5);
        if (fabs_(q1) > fabs_(q2)) { r[0] = dvd(q1, a1); r[1] = dvd(a3, q1); }
        else { r[0] = dvd(q2, a1); r[1] = dvd(a3, q2); }
        return d > 0 ? 2 : 1;
    }
    a0 = dvd(1.0, a0);
    a1 = mul(a1, a0); a2 = mul(a2, a0); a3 = mul(a3, a0);
    if (!(sub(a1, a1) == 0 && sub(a2, a2) == 0 && sub(a3, a3) == 0)) return 0;  // not finite
    const double Q = mul(sub(mul(a1, a1), mul(3.0, a2)), 1.0 / 9);
    const double d = mul(sub(add(mul(mul(a1, a1), sub(mul(a2, a2), mul(mul(4.0, a1), a3))), mul(mul(2.0, a2), sub(mul(mul(9.0, a1), a3), mul(mul(2.0, a2), a2)))),
                             mul(mul(27.0, a3), a3)),
                         1.0 / 108);
    double B = fabs_(a1);
    if (fabs_(a2) > B) B = fabs_(a2);
    if (fabs_(a3) > B) B = fabs_(a3);
    B = add(B, 1.0);  // Cauchy bound of every root
    if (d > 0 && Q > 0) {
        const double sq = sqr(Q), m = dvd(-a1, 3.0);
        const double m1 = sub(m, sq), m2 = add(m, sq);
        r[0] = bisect(a1, a2, a3, -B, m1, true);
        r[1] = bisect(a1, a2, a3, m1, m2, false);
        r[2] = bisect(a1, a2, a3, m2, B, true);
        return 3;
    }
    r[0] = bisect(a1, a2, a3, -B, B, true);
    return 1;
}

// run7Point: up to three fundamental matrices (row-major, F[8] = 1 or 0) through the 7 correspondences (x0, y0) <-> (x1, y1)
FM_HD int run7point(const float *x0f, const float *y0f, const float *x1f, const float *y1f, double *F /* [3][9] */)
{
    double a[7][9];  // a[i] = row i of the 7 x 9 system = column i of its transpose
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const double x0 = x0f[i], y0 = y0f[i], x1 = x1f[i], y1 = y1f[i];
        a[i][0] = mul(x1, x0); a[i][1] = mul(x1, y0); a[i][2] = x1;
        a[i][3] = mul(y1, x0); a[i][4] = mul(y1, y0); a[i][5] = y1;
        a[i][6] = x0; a[i][7] = y0; a[i][8] = 1.0;
    }
    // Householder QR of A^T (9 x 7): reflection k zeroes rows k+1..8 of column k; v_k overwrites a[k][k..8]
    double beta[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        double nrm2 = 0.0;
#pragma unroll
        for (int r = k; r < 9; r++) nrm2 = add(nrm2, mul(a[k][r], a[k][r]));
        if (nrm2 == 0.0) { beta[k] = 0.0; continue; }
        const double nrm = sqr(nrm2);
        a[k][k] = a[k][k] >= 0 ? add(a[k][k], nrm) : sub(a[k][k], nrm);  // x0 - alpha, alpha = -sign(x0) |x|
        double vtv = 0.0;
#pragma unroll
        for (int r = k; r < 9; r++) vtv = add(vtv, mul(a[k][r], a[k][r]));
        beta[k] = dvd(2.0, vtv);
#pragma unroll
        for (int c = k + 1; c < 7; c++) {
            double w = 0.0;
#pragma unroll
            for (int r = k; r < 9; r++) w = add(w, mul(a[k][r], a[c][r]));
            w = mul(w, beta[k]);
#pragma unroll
            for (int r = k; r < 9; r++) a[c][r] = sub(a[c][r], mul(w, a[k][r]));
        }
    }
    // f1 = Q e7, f2 = Q e8 (Q = H0 H1 ... H6): the null space of the system
    double f1[9], f2[9];
#pragma unroll
    for (int r = 0; r < 9; r++) { f1[r] = r == 7 ? 1.0 : 0.0; f2[r] = r == 8 ? 1.0 : 0.0; }
#pragma unroll
    for (int k = 6; k >= 0; k--) {
        if (beta[k] == 0.0) continue;
        double w1 = 0.0, w2 = 0.0;
#pragma unroll
        for (int r = k; r < 9; r++) { w1 = add(w1, mul(a[k][r], f1[r])); w2 = add(w2, mul(a[k][r], f2[r])); }
        w1 = mul(w1, beta[k]); w2 = mul(w2, beta[k]);
#pragma unroll
        for (int r = k; r < 9; r++) { f1[r] = sub(f1[r], mul(w1, a[k][r])); f2[r] = sub(f2[r], mul(w2, a[k][r])); }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) f1[i] = sub(f1[i], f2[i]);
    // det(l f1 + f2) = c0 l^3 + c1 l^2 + c2 l + c3: run7Point's expressions, left to right
    auto m2 = [](double p, double q, double r, double s) { return sub(mul(p, q), mul(r, s)); };
    double c[4], t0, t1, t2;
    t0 = m2(f2[4], f2[8], f2[5], f2[7]); t1 = m2(f2[3], f2[8], f2[5], f2[6]); t2 = m2(f2[3], f2[7], f2[4], f2[6]);
    c[3] = add(sub(mul(f2[0], t0), mul(f2[1], t1)), mul(f2[2], t2));
    c[2] = add(sub(add(sub(add(sub(add(sub(mul(f1[0], t0), mul(f1[1], t1)), mul(f1[2], t2)), mul(f1[3], m2(f2[1], f2[8], f2[2], f2[7]))),
                                   mul(f1[4], m2(f2[0], f2[8], f2[2], f2[6]))),
                               mul(f1[5], m2(f2[0], f2[7], f2[1], f2[6]))),
                           mul(f1[6], m2(f2[1], f2[5], f2[2], f2[4]))),
                       mul(f1[7], m2(f2[0], f2[5], f2[2], f2[3]))),
               mul(f1[8], m2(f2[0], f2[4], f2[1], f2[3])));
    t0 = m2(f1[4], f1[8], f1[5], f1[7]); t1 = m2(f1[3], f1[8], f1[5], f1[6]); t2 = m2(f1[3], f1[7], f1[4], f1[6]);
    c[1] = add(sub(add(sub(add(sub(add(sub(mul(f2[0], t0), mul(f2[1], t1)), mul(f2[2], t2)), mul(f2[3], m2(f1[1], f1[8], f1[2], f1[7]))),
                                   mul(f2[4], m2(f1[0], f1[8], f1[2], f1[6]))),
                               mul(f2[5], m2(f1[0], f1[7], f1[1], f1[6]))),
                           mul(f2[6], m2(f1[1], f1[5], f1[2], f1[4]))),
                       mul(f2[7], m2(f1[0], f1[5], f1[2], f1[3]))),
               mul(f2[8], m2(f1[0], f1[4], f1[1], f1[3])));
    c[0] = add(sub(mul(f1[0], t0), mul(f1[1], t1)), mul(f1[2], t2));
    double r[3] = {0.0, 0.0, 0.0};
    const int n = solve_cubic(c, r);
    if (n < 1 || n > 3) return 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (k >= n) break;
        double lambda = r[k], mu = 1.0;
        const double s = add(mul(f1[8], r[k]), f2[8]);
        double *Fk = F + 9 * k;
        if (fabs_(s) > kDblEpsilon) {
            mu = dvd(1.0, s);
            lambda = mul(lambda, mu);
            Fk[8] = 1.0;
        } else {
            Fk[8] = 0.0;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) Fk[i] = add(mul(f1[i], lambda), mul(f2[i], mu));
    }
    return n;
}

// natural log of a positive normal double: x = m 2^e (m in [sqrt(1/2), sqrt(2))), log m = 2 atanh(s), s = (m - 1) / (m + 1)
FM_HD double log_(double x)
{
    int e = 0;
    double m = frexp(x, &e);
    if (m < kSqrtHalf) { m = mul(m, 2.0); e -= 1; }
    const double s = dvd(sub(m, 1.0), add(m, 1.0)), z = mul(s, s);
    double acc = 1.0 / 23;
    acc = add(mul(acc, z), 1.0 / 21); acc = add(mul(acc, z), 1.0 / 19); acc = add(mul(acc, z), 1.0 / 17);
    acc = add(mul(acc, z), 1.0 / 15); acc = add(mul(acc, z), 1.0 / 13); acc = add(mul(acc, z), 1.0 / 11);
    acc = add(mul(acc, z), 1.0 / 9); acc = add(mul(acc, z), 1.0 / 7); acc = add(mul(acc, z), 1.0 / 5);
    acc = add(mul(acc, z), 1.0 / 3); acc = add(mul(acc, z), 1.0);
    return add(mul((double)e, kLn2), mul(mul(2.0, s), acc));
}

// cvRound: nearest integer, ties to even (x >= 0 here)
FM_HD int round_even(double x)
{
    const double f = floor(x), d = sub(x, f);
    long long r = (long long)f;
    if (d > 0.5 || (d == 0.5 && (r & 1))) r++;
    return (int)r;
}

// RANSACUpdateNumIters(p, ep, modelPoints, maxIters); (1 - ep)^modelPoints as a fixed multiplication chain: 7 -> ((q^2 q)^2) q, 4 -> q^2 q^2
FM_HD int update_num_iters(double p, double ep, int maxIters, int modelPoints = kModelPoints)
{
    p = p < 0 ? 0 : (p > 1 ? 1 : p);
    ep = ep < 0 ? 0 : (ep > 1 ? 1 : ep);
    double num = sub(1.0, p);
    if (num < kDblMin) num = kDblMin;
    const double q = sub(1.0, ep), q2 = mul(q, q), q3 = mul(q2, q), q6 = mul(q3, q3), q7 = mul(q6, q);
    double denom = sub(1.0, modelPoints == 4 ? mul(q2, q2) : q7);
    if (denom < kDblMin) return 0;
    num = log_(num);
    denom = log_(denom);
    return (denom >= 0 || -num >= mul((double)maxIters, -denom)) ? maxIters : round_even(dvd(num, denom));
}

// FMEstimatorCallback::computeError for one correspondence: (float) std::max(d1^2 s1, d2^2 s2), doubles left to right
FM_HD float point_error(const double *F, float x1f, float y1f, float x2f, float y2f)
{
    const double x1 = x1f, y1 = y1f, x2 = x2f, y2 = y2f;
    double a = add(add(mul(F[0], x1), mul(F[1], y1)), F[2]);
    double b = add(add(mul(F[3], x1), mul(F[4], y1)), F[5]);
    double c = add(add(mul(F[6], x1), mul(F[7], y1)), F[8]);
    const double s2 = dvd(1.0, add(mul(a, a), mul(b, b)));
    const double d2 = add(add(mul(x2, a), mul(y2, b)), c);
    a = add(add(mul(F[0], x2), mul(F[3], y2)), F[6]);
    b = add(add(mul(F[1], x2), mul(F[4], y2)), F[7]);
    c = add(add(mul(F[2], x2), mul(F[5], y2)), F[8]);
    const double s1 = dvd(1.0, add(mul(a, a), mul(b, b)));
    const double d1 = add(add(mul(x1, a), mul(y1, b)), c);
    const double e1 = mul(mul(d1, d1), s1), e2 = mul(mul(d2, d2), s2);
    return (float)(e1 < e2 ? e2 : e1);
}

}  // namespace fm
}  // namespace amos
