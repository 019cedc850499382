// amos_sim3_core.h -- the pieces of ORB-SLAM2's Sim3Solver (src/Sim3Solver.cc:48-523: SetRansacParameters, the three draws of iterate,
// ComputeSim3 after Horn 1987, CheckInliers / Project / FromCameraToImage), written once for host and device.  Included by amos_sim3.hip
// (k_sim3_iterate: one hypothesis per lane); tests/host_sim3 compiles it as plain C++ into a complete single-threaded solver.
// tests/sim3_restatement.py is the same arithmetic in Python float32 / float64 and the tests hold both compilations to it bit for bit:
// every operation is rounded on its own, in source order (explicit _rn operations on the device, -ffp-contract=off on the host).
// PARITY WITH THE REFERENCE'S OPENCV-BACKED ARITHMETIC IS UNPINNED (cv::eigen runs in float, cv::Rodrigues and atan2 are library code).
// The conventions that fix each cv::Mat expression:
//   A * B, A * B + C, a * A * B     one gemm: the products widened to double and summed left to right (no leading zero), C or the scalar
//                                   applied in double, ONE rounding to float (the rule of gemm_row, amos_scene_flow.h)
//   s * A, A / n                    one float32 product per element with (float) s, (float)(1.0 / n)
//   (1.0 / s) * A                   the same with (float)(1.0 / (double) s)
//   -A * b                          the gemm's double sum negated, one rounding
//   cv::reduce(SUM), A - B          float32, left to right
//   Mat::dot, the loop of :407-413  a double accumulator from 0.0 over the float32 products in row-major order (ComputeSim3's nom, den);
//                                   CheckInliers' dist.dot(dist) of two terms is the float32 sum of the two float32 squares
//   cv::eigen(N)                    pnp::jacobi_sym in double on the 4 x 4 matrix of the ten float32 entries; the eigenvector of the largest
//                                   eigenvalue, the FIRST of equal ones in jacobi_sym's output order
//   atan2 / angle-axis / Rodrigues  mathematically the rotation matrix of the normalised quaternion, whatever the eigenvector's sign:
//                                   R from q / |q| in double with + - * / sqrt, one rounding to float per entry
// Where the imaginary part of q has norm exactly 0 (pure translation, coincident samples) the reference divides 0 / 0 and scores a NaN
// rotation: there THE HYPOTHESIS HAS NO INLIERS; its R (the identity), t and s are what the formulas give.  NaN and infinity may arise
// elsewhere (collinear samples, den == 0, z == 0) and fail every inlier test on their own; a NaN leaves sim3_horn as the quiet NaN
// 0x7FC00000 so that host, device and Python store the same bytes.  The acceptance bound is (float)(9.210 * (double) sigma2).
#pragma once

#include "amos_pnp_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace amos {
namespace sim3 {

using pnp::fadd;
using pnp::fmul;
using pnp::fsub;

constexpr int kMaxCorrespondences = 2048;

#if defined(__HIP_DEVICE_COMPILE__)
FM_HD float fdiv(float a, float b) { return __fdiv_rn(a, b); }
#else
FM_HD float fdiv(float a, float b) { return a / b; }
#endif

FM_HD float canon(float x) { return x != x ? __builtin_nanf("") : x; }

// SetRansacParameters (Sim3Solver.cc:143-196): the adjusted mRansacMaxIts for N correspondences
FM_HD int sim3_parameters(int N, double probability, int minInliers, int maxIterations)
{
    int nIt = minInliers == N ? 1 : pnp::solver_iterations(fdiv((float)minInliers, (float)N), probability, maxIterations);
    nIt = nIt < maxIterations ? nIt : maxIterations;
    return nIt > 1 ? nIt : 1;
}

// the three swap-with-back draws of one iteration (:228-249): every iteration consumes exactly three draws
FM_HD void sim3_draw3(uint64_t &rng, int N, int *idx) { pnp::solver_draw<3>(rng, N, idx); }
// the same from the generator's outputs drawn ahead: next() hands them out in order
template <class Next>
FM_HD void sim3_draw3_of(Next next, int N, int *idx) { pnp::solver_draw_of<3>(next, N, idx); }

FM_HD float max_error(float sigma2) { return (float)fm::mul(9.210, (double)sigma2); }

// one row of a gemm: (float)(a0 b0 + a1 b1 + a2 b2 [+ c])
FM_HD double dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return fm::add(fm::add(fm::mul((double)a0, (double)b0), fm::mul((double)a1, (double)b1)), fm::mul((double)a2, (double)b2));
}
FM_HD float gemm3(const float *R, int r, float x, float y, float z, float t)
{
    return (float)fm::add(dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], x, y, z), (double)t);
}

// X3Dc = Rcw * Xw + tcw (:118-122)
FM_HD void to_camera(const float *Rcw, const float *tcw, const float *Xw, float *Xc)
{
    for (int r = 0; r < 3; r++) Xc[r] = gemm3(Rcw, r, Xw[0], Xw[1], Xw[2], tcw[r]);
}

// FromCameraToImage / the tail of Project (:517-521, :538-543)
FM_HD void to_image(float X, float Y, float Z, float fx, float fy, float cx, float cy, float &u, float &v)
{
    const float invz = fdiv(1.0f, Z), x = fmul(X, invz), y = fmul(Y, invz);
    u = fadd(fmul(fx, x), cx);
    v = fadd(fmul(fy, y), cy);
}

struct Hypothesis {
    float R[9], t[3], s;     // mR12i, mt12i, ms12i
    float sR[9];             // T12 = [sR | t]
    float sRi[9], ti[3];     // T21 = [sRi | ti]
    int degenerate;          // |Im q| == 0: no inliers
};

// ComputeSim3 (:309-448).  P[r][c]: coordinate r of sample c
FM_HD void sim3_horn(const float (&P1)[3][3], const float (&P2)[3][3], bool fixScale, Hypothesis &h)
{
    const float third = (float)(1.0 / 3.0);
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        O1[r] = fmul(fadd(fadd(P1[r][0], P1[r][1]), P1[r][2]), third);
        O2[r] = fmul(fadd(fadd(P2[r][0], P2[r][1]), P2[r][2]), third);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            Pr1[r][c] = fsub(P1[r][c], O1[r]);
            Pr2[r][c] = fsub(P2[r][c], O2[r]);
        }
    }
    float M[3][3];  // Pr2 * Pr1^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = (float)dot3(Pr2[i][0], Pr2[i][1], Pr2[i][2], Pr1[j][0], Pr1[j][1], Pr1[j][2]);
    const float N11 = fadd(fadd(M[0][0], M[1][1]), M[2][2]), N12 = fsub(M[1][2], M[2][1]), N13 = fsub(M[2][0], M[0][2]),
                N14 = fsub(M[0][1], M[1][0]), N22 = fsub(fsub(M[0][0], M[1][1]), M[2][2]), N23 = fadd(M[0][1], M[1][0]),
                N24 = fadd(M[2][0], M[0][2]), N33 = fsub(fadd(-M[0][0], M[1][1]), M[2][2]), N34 = fadd(M[1][2], M[2][1]),
                N44 = fadd(fsub(-M[0][0], M[1][1]), M[2][2]);
    double A[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44}, V[16];
    pnp::jacobi_sym(A, V, 4);
    double lam = A[0], q0 = V[0], q1 = V[4], q2 = V[8], q3 = V[12];
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (A[5 * i] > lam) { lam = A[5 * i]; q0 = V[i]; q1 = V[4 + i]; q2 = V[8 + i]; q3 = V[12 + i]; }
    const double imag = fm::add(fm::add(fm::mul(q1, q1), fm::mul(q2, q2)), fm::mul(q3, q3));
    h.degenerate = imag == 0 ? 1 : 0;
    const double nq = fm::sqr(fm::add(fm::mul(q0, q0), imag));
    const double a = fm::dvd(q0, nq), b = fm::dvd(q1, nq), c = fm::dvd(q2, nq), d = fm::dvd(q3, nq);
    const double bb = fm::mul(b, b), cc = fm::mul(c, c), dd = fm::mul(d, d), bc = fm::mul(b, c), bd = fm::mul(b, d), cd = fm::mul(c, d),
                 ab = fm::mul(a, b), ac = fm::mul(a, c), ad = fm::mul(a, d);
    float R[9];
    R[0] = (float)fm::sub(1.0, fm::mul(2.0, fm::add(cc, dd)));
    R[1] = (float)fm::mul(2.0, fm::sub(bc, ad));
    R[2] = (float)fm::mul(2.0, fm::add(bd, ac));
    R[3] = (float)fm::mul(2.0, fm::add(bc, ad));
    R[4] = (float)fm::sub(1.0, fm::mul(2.0, fm::add(bb, dd)));
    R[5] = (float)fm::mul(2.0, fm::sub(cd, ab));
    R[6] = (float)fm::mul(2.0, fm::sub(bd, ac));
    R[7] = (float)fm::mul(2.0, fm::add(cd, ab));
    R[8] = (float)fm::sub(1.0, fm::mul(2.0, fm::add(bb, cc)));
    float s = 1.0f;
    if (!fixScale) {  // P3 = R * Pr2; nom = Pr1 . P3, den = sum of P3^2
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float p3 = (float)dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], Pr2[0][j], Pr2[1][j], Pr2[2][j]);
                nom = fm::add(nom, (double)fmul(Pr1[i][j], p3));
                den = fm::add(den, (double)fmul(p3, p3));
            }
        s = (float)fm::dvd(nom, den);
    }
    const float inv = (float)fm::dvd(1.0, (double)s);
    float t[3];
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] = (float)fm::sub((double)O1[r], fm::mul((double)s, dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], O2[0], O2[1], O2[2])));
    float sRi[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c2 = 0; c2 < 3; c2++) sRi[3 * r + c2] = fmul(inv, R[3 * c2 + r]);
#pragma unroll
    for (int r = 0; r < 3; r++) h.ti[r] = canon((float)-dot3(sRi[3 * r], sRi[3 * r + 1], sRi[3 * r + 2], t[0], t[1], t[2]));
#pragma unroll
    for (int k = 0; k < 9; k++) {
        h.R[k] = canon(R[k]);
        h.sR[k] = canon(fmul(s, R[k]));
        h.sRi[k] = canon(sRi[k]);
    }
#pragma unroll
    for (int r = 0; r < 3; r++) h.t[r] = canon(t[r]);
    h.s = canon(s);
}

// one correspondence as the constructor leaves it: X3Dc1, X3Dc2, mvP1im1, mvP2im2, mvnMaxError1 / 2
struct Correspondence {
    float X1[3], X2[3], p1[2], p2[2], maxErr1, maxErr2;
};

// CheckInliers (:451-479) for one correspondence; K1 / K2: fx, fy, cx, cy
FM_HD bool sim3_inlier(const Hypothesis &h, const Correspondence &c, const float *K1, const float *K2)
{
    float u, v;
    to_image(gemm3(h.sR, 0, c.X2[0], c.X2[1], c.X2[2], h.t[0]), gemm3(h.sR, 1, c.X2[0], c.X2[1], c.X2[2], h.t[1]),
             gemm3(h.sR, 2, c.X2[0], c.X2[1], c.X2[2], h.t[2]), K1[0], K1[1], K1[2], K1[3], u, v);
    const float d1x = fsub(c.p1[0], u), d1y = fsub(c.p1[1], v), err1 = fadd(fmul(d1x, d1x), fmul(d1y, d1y));
    to_image(gemm3(h.sRi, 0, c.X1[0], c.X1[1], c.X1[2], h.ti[0]), gemm3(h.sRi, 1, c.X1[0], c.X1[1], c.X1[2], h.ti[1]),
             gemm3(h.sRi, 2, c.X1[0], c.X1[1], c.X1[2], h.ti[2]), K2[0], K2[1], K2[2], K2[3], u, v);
    const float d2x = fsub(u, c.p2[0]), d2y = fsub(v, c.p2[1]), err2 = fadd(fmul(d2x, d2x), fmul(d2y, d2y));
    return !h.degenerate && err1 < c.maxErr1 && err2 < c.maxErr2;
}

// mT12i: [sR | t] over 0 0 0 1
FM_HD void sim3_T12(const Hypothesis &h, float *T)
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[4 * r + c] = h.sR[3 * r + c];
        T[4 * r + 3] = h.t[r];
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
}

}  // namespace sim3
}  // namespace amos
